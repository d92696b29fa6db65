// gnnb_k_frontier.h -- the per-round steps of a branch-and-bound loop whose open domains stay in device memory:
// gnnb_frontier_gather, gnnb_frontier_expand, gnnb_frontier_commit (and, at the end of this file, the BaBSR fall-back below
// a branching threshold of section 7.5: gnnb_frontier_fallback, gnnb_frontier_choose, their many-job form of section 7.6, and the selection
// of the rows an online round learns from, section 7.7: gnnb_frontier_learn, per job of a pool, section 7.19: gnnb_frontier_learn_jobs; the witness of the upper bound, section 7.8:
// gnnb_frontier_witness; BaBSR alone in the GNN's place, section 7.10: gnnb_frontier_babsr_decide; and a round that splits each parent on
// several ReLUs, section 7.20: gnnb_frontier_expand_depth, gnnb_frontier_commit_depth).  Between them run the existing
// batch kernels (gnnb_dual_ascent at n_iter = 0 for the scorer's inputs, gnnb_forward, gnnb_kw_bounds, gnnb_dual_ascent), untouched, and
// the network's value at a round's points: gnnb_net_eval or the descent that can take its place, gnnb_net_descend (gnnb_k_net.h).
//
// The POOL is a struct of arrays over `capacity` slots: mask (cap, R) int8, the fp64 bounds of graph layers 1..L+1 (cap, N_k) exactly as
// gnnb_kw_bounds wrote them, the best dual point alpha / beta (cap, R), its value bound (cap) and the flag open (cap).
//
//   * k_frontier_gather   pool rows of K slots -> dense batch rows: mask, bounds, alpha / beta, the fp32 roundings of the bounds
//                         (layer 0 = the box), the scorer's mask (1.0 where the pool mask is -1).  Plain copies.
//   * k_frontier_expand   K parents + gnnb_forward's decisions -> 2K child rows (2i blocked, 2i + 1 passing): the parent's mask with
//                         one entry set, the parent's bounds as gnnb_kw_bounds' parent tables, split_layer, the parent's dual point,
//                         live.  A parent without a decision ([-1, -1]) yields two complete rows with live = 0 (the batch kernels
//                         behind run on them like on any other row; commit ignores them).
//   * k_frontier_resolve  per child: the mask resolved by the bounds (-1 with lo >= 0 -> 1, -1 with up <= 0 -> 0) and whether an
//                         undecided node is left.
//   * k_frontier_decide   ONE workgroup: global_ub, keep or close every child, the parents' slots freed, the kept children's
//                         destination slots by a prefix sum over the 2K keep flags in child order, the state record (fr_decide on
//                         the view of the whole pool; k_frontier_decide_jobs at the end of this file runs it per job on a segment).
//   * k_frontier_store    kept children -> their pool slots.
//
// The arrays of a set of domains -- the pool's slots, a round's child rows -- are one struct, FrDomainsT (FrChildrenT adds what a bounded
// child has: infeasible, bound, ubv, live; FrPool what a slot has: bound, open), writable or read-only by its parameter, and fr_copy_row
// is the one copy of a row between two sets: k_frontier_expand, k_frontier_store and k_frontier_choose_copy call it.
//
// A kept child of rank r (its number among the kept ones, in child order) goes to the r-th parent slot in the order of `slots`; from
// rank K on to slot in_use + (r - K), in_use the state record's count before the call.  No atomics, no workgroup waits on another;
// minima and counts are per-thread partials in a fixed order, then a fixed tree: nothing depends on K or on a row's place.

#define FR_THREADS KW_THREADS
#define FR_SPLIT 8              // workgroups a row of the copy kernels is spread over

// the state record (device, doubles; counts are whole numbers)
enum { FS_GLOBAL_UB, FS_CLOSED_LB, FS_LOWEST_OPEN, FS_N_OPEN, FS_IN_USE, FS_KEPT, FS_CLOSED, FS_INFEASIBLE, FS_OVERFLOW, FS_COUNT };
static_assert(FS_COUNT == GNNB_FRONTIER_STATE_DOUBLES, "include/gnnb.h: the state record");

struct FrShape {                // the sizes the copy kernels need of the bound network
  int N[MAXL + 2], off[MAXL + 2];                       // graph layers 0..L+1; off[k]: flat ReLU index of layer k's first node
  int L, R;
};

// The arrays of a set of domains, one row per domain -- the pool's slots, a round's child rows -- and what child rows add to them.  Q makes
// the element types: FrRW for a set a kernel writes, FrRO for one it only reads.
template <class T> using FrRW = T;
template <class T> using FrRO = const T;

template <template <class> class Q> struct FrDomainsT {
  Q<int8_t>* mask; Q<double>* lb[MAXL + 2]; Q<double>* ub[MAXL + 2];     // lb / ub: graph layers 1..L+1
  Q<double>* alpha; Q<double>* beta;
};
template <template <class> class Q> struct FrChildrenT : FrDomainsT<Q> {  // gnnb_children / gnnb_children_rw
  Q<int32_t>* infeasible; Q<double>* bound; Q<double>* ubv; Q<int32_t>* live;
};
using FrDomains = FrDomainsT<FrRW>;
using FrChildren = FrChildrenT<FrRW>;
using FrChildrenRO = FrChildrenT<FrRO>;

struct FrPool : FrDomains {
  double* bound; int32_t* open;
  int cap;
};

struct FrGatherArgs {
  FrShape s; FrPool p;
  const int32_t* slots; int K;
  const double* x_lo; const double* x_hi;               // (K, N_0)
  int8_t* mask; double* lb[MAXL + 2]; double* ub[MAXL + 2];
  float* lb32[MAXL + 2]; float* ub32[MAXL + 2];         // graph layers 0..L+1
  double* alpha; double* beta; float* amb;
};

struct FrExpandArgs {
  FrShape s; FrPool p;
  const int32_t* slots; const int32_t* decisions; int K;
  FrDomains ch;                                         // the 2K children; lb / ub: gnnb_kw_bounds' parent tables
  int32_t* split; int32_t* live;
};

struct FrCommitArgs {
  FrShape s; FrPool p;
  const int32_t* slots; int K;
  FrChildrenRO ch;                                      // the 2K children
  double eps, decision_bound;
  double* state;
  int8_t* rmask; int32_t* undecided; int32_t* dest;     // workspace: (2K, R), (2K), (2K)
};
static_assert(sizeof(FrGatherArgs) <= 4096 && sizeof(FrExpandArgs) <= 4096 && sizeof(FrCommitArgs) <= 4096, "kernel arguments: 4 KiB");

__device__ __forceinline__ bool fr_slot_ok(const FrPool& p, int s) { return s >= 0 && s < p.cap; }

// Row c of `src` to row d of `dst`: mask / alpha / beta over the R ReLU nodes, lb / ub of graph layers 1..L+1, the row spread over the
// FR_SPLIT workgroups of blockIdx.y.  mask: the source of the mask's row (src.mask, or the resolved masks of a commit).
template <template <class> class Q>
__device__ __forceinline__ void fr_copy_row(const FrShape& s, const FrDomains& dst, long d, const FrDomainsT<Q>& src, const int8_t* mask, long c) {
  const int t0 = blockIdx.y * FR_THREADS + threadIdx.x, dt = FR_SPLIT * FR_THREADS;
  const int R = s.R, K1 = s.L + 1;
  for (int r = t0; r < R; r += dt) {
    dst.mask[d * R + r] = mask[c * R + r];
    dst.alpha[d * R + r] = src.alpha[c * R + r];
    dst.beta[d * R + r] = src.beta[c * R + r];
  }
  for (int k = 1; k <= K1; ++k) {
    const int Nk = s.N[k];
    for (int j = t0; j < Nk; j += dt) {
      dst.lb[k][d * Nk + j] = src.lb[k][c * Nk + j];
      dst.ub[k][d * Nk + j] = src.ub[k][c * Nk + j];
    }
  }
}

__global__ __launch_bounds__(FR_THREADS) void k_frontier_gather(FrGatherArgs a) {
  const int i = blockIdx.x, t0 = blockIdx.y * FR_THREADS + threadIdx.x, dt = FR_SPLIT * FR_THREADS;
  const int s = a.slots[i];
  if (!fr_slot_ok(a.p, s)) return;                      // (a slot outside the pool leaves its row as it is)
  const int R = a.s.R, K1 = a.s.L + 1;
  for (int r = t0; r < R; r += dt) {
    const int8_t m = a.p.mask[(long)s * R + r];
    a.mask[(long)i * R + r] = m;
    a.amb[(long)i * R + r] = m == -1 ? 1.0f : 0.0f;
    a.alpha[(long)i * R + r] = a.p.alpha[(long)s * R + r];
    a.beta[(long)i * R + r] = a.p.beta[(long)s * R + r];
  }
  for (int j = t0; j < a.s.N[0]; j += dt) {
    a.lb32[0][(long)i * a.s.N[0] + j] = (float)a.x_lo[(long)i * a.s.N[0] + j];
    a.ub32[0][(long)i * a.s.N[0] + j] = (float)a.x_hi[(long)i * a.s.N[0] + j];
  }
  for (int k = 1; k <= K1; ++k) {
    const int Nk = a.s.N[k];
    for (int j = t0; j < Nk; j += dt) {
      const double l = a.p.lb[k][(long)s * Nk + j], u = a.p.ub[k][(long)s * Nk + j];
      a.lb[k][(long)i * Nk + j] = l;
      a.ub[k][(long)i * Nk + j] = u;
      a.lb32[k][(long)i * Nk + j] = (float)l;
      a.ub32[k][(long)i * Nk + j] = (float)u;
    }
  }
}

__global__ __launch_bounds__(FR_THREADS) void k_frontier_expand(FrExpandArgs a) {
  const int c = blockIdx.x, i = c >> 1, choice = c & 1, t0 = blockIdx.y * FR_THREADS + threadIdx.x, dt = FR_SPLIT * FR_THREADS;
  const int s = a.slots[i];
  if (!fr_slot_ok(a.p, s)) {                            // no such parent: a dead row nobody reads
    if (t0 == 0) { a.live[c] = 0; a.split[c] = -1; }
    return;
  }
  const int lay = a.decisions[2 * i], idx = a.decisions[2 * i + 1];
  const bool live = lay >= 0 && lay < a.s.L && idx >= 0 && idx < a.s.N[lay + 1];
  const int node = live ? a.s.off[lay + 1] + idx : -1;
  fr_copy_row(a.s, a.ch, c, a.p, a.p.mask, s);
  if (live && node % dt == t0) a.ch.mask[(long)c * a.s.R + node] = (int8_t)choice;      // by the thread that copied the entry: no second pass
  if (t0 == 0) {
    a.live[c] = live ? 1 : 0;
    a.split[c] = live ? lay : a.s.L - 1;                // a dead row keeps every bound of its parent
  }
}

__global__ __launch_bounds__(FR_THREADS) void k_frontier_resolve(FrCommitArgs a) {
  const int c = blockIdx.x, tid = threadIdx.x, R = a.s.R;
  int open = 0;
  if (a.ch.live[c]) {                                   // (a dead row's arrays are never read)
    for (int k = 1; k <= a.s.L; ++k) {
      const int Nk = a.s.N[k];
      for (int j = tid; j < Nk; j += FR_THREADS) {
        const long r = (long)c * R + a.s.off[k] + j;
        int m = a.ch.mask[r];
        if (m == -1 && a.ch.lb[k][(long)c * Nk + j] >= 0.0) m = 1;
        if (m == -1 && a.ch.ub[k][(long)c * Nk + j] <= 0.0) m = 0;
        a.rmask[r] = (int8_t)m;
        open |= m == -1;
      }
    }
  }
  open = __syncthreads_or(open);
  if (tid == 0) a.undecided[c] = open ? 1 : 0;
}

// min / sum of one value per thread over the workgroup, on every thread (fixed tree)
__device__ __forceinline__ double fr_block_min(double* red, double v, int tid) {
  __syncthreads();
  red[tid] = v;
  __syncthreads();
  for (int s = FR_THREADS / 2; s > 0; s >>= 1) {
    if (tid < s) red[tid] = fmin(red[tid], red[tid + s]);
    __syncthreads();
  }
  const double out = red[0];
  __syncthreads();
  return out;
}

// What one job's commit sees of the pool and the children: the slots [base, base + cap) (in_use and every destination above the parents'
// slots count from base), the parents' rows [row0, row0 + K) of `slots`, their children [2 row0, 2 row0 + 2K), the job's record and
// decision bound.  k_frontier_decide is the view {0, pool capacity, 0, K, state, decision_bound}.  With C children per parent (fr_decide's
// argument; 2 but for a round of section 7.20) the children are rows [C row0, C row0 + C K).
struct FrView {
  int base, cap, row0, K;
  double* state;
  double decision_bound;
};

__device__ __forceinline__ bool fr_view_ok(const FrView& v, int s) { return s >= v.base && s < v.base + v.cap; }

// global_ub, keep or close every child of the view, its parents' slots freed, the kept children's destination slots by a prefix sum
// over the C K keep flags in child order, the record.  C: the children per parent (parent i's are rows C i .. C i + C - 1).  One
// workgroup; red: FR_THREADS doubles, cnt: FR_THREADS + 1 ints of LDS.
__device__ __forceinline__ void fr_decide(const FrCommitArgs& a, const FrView& v, int C, double* red, int* cnt) {
  const int tid = threadIdx.x, K = v.K, n = C * K;
  const int32_t* slots = a.slots + v.row0;
  const long ch0 = (long)C * v.row0;                    // the view's first child row
  const double inf = __longlong_as_double(0x7ff0000000000000LL);
  const int in_use = min(max((int)v.state[FS_IN_USE], 0), v.cap);
  // 2. the incumbent: every live feasible child's network value at its LP point
  double val = inf;
  for (int c = tid; c < n; c += FR_THREADS)
    if (a.ch.live[ch0 + c] && !a.ch.infeasible[ch0 + c]) val = fmin(val, a.ch.ubv[ch0 + c]);
  const double gub = fmin(v.state[FS_GLOBAL_UB], fr_block_min(red, val, tid));
  // 3. - 5. keep or close (each thread a contiguous run of children, so that ranks follow child order)
  const int per = (n + FR_THREADS - 1) / FR_THREADS, c0 = min(tid * per, n), c1 = min(c0 + per, n);
  const bool have_db = v.decision_bound == v.decision_bound;
  double closed = inf;
  int kept = 0, n_closed = 0, n_inf = 0;
  for (int c = c0; c < c1; ++c) {
    if (!a.ch.live[ch0 + c]) continue;
    if (a.ch.infeasible[ch0 + c]) { ++n_inf; continue; }
    const double lb = a.ch.bound[ch0 + c];
    if (a.undecided[ch0 + c] && lb < gub - a.eps && (!have_db || lb < v.decision_bound)) ++kept;
    else { closed = fmin(closed, lb); ++n_closed; }
  }
  for (int i = tid; i < K; i += FR_THREADS) {           // a parent without a live child (decision [-1, -1]) is closed at its own bound
    const int s = slots[i];
    if (!fr_view_ok(v, s)) continue;
    int live = 0;
    for (int j = 0; j < C; ++j) live |= a.ch.live[ch0 + (long)C * i + j];
    if (!live) { closed = fmin(closed, a.p.bound[s]); ++n_closed; }
  }
  // 6. the parents leave the pool
  for (int i = tid; i < K; i += FR_THREADS)
    if (fr_view_ok(v, slots[i])) a.p.open[slots[i]] = 0;
  // 7. ranks of the kept children: exclusive prefix sum of the per-thread counts
  cnt[tid + 1] = kept;
  if (tid == 0) cnt[0] = 0;
  __syncthreads();                                      // (also: every open[] = 0 above is visible below)
  if (tid == 0)
    for (int t = 1; t <= FR_THREADS; ++t) cnt[t] += cnt[t - 1];
  __syncthreads();
  int rank = cnt[tid], top = 0, dropped = 0;
  const int total_kept = cnt[FR_THREADS];
  for (int c = c0; c < c1; ++c) {
    int d = -1;
    if (a.ch.live[ch0 + c] && !a.ch.infeasible[ch0 + c]) {
      const double lb = a.ch.bound[ch0 + c];
      if (a.undecided[ch0 + c] && lb < gub - a.eps && (!have_db || lb < v.decision_bound)) {
        d = rank < K ? slots[rank] : v.base + in_use + (rank - K);
        ++rank;
        if (!fr_view_ok(v, d)) {                        // no room (the caller checks the capacity before a round): the bound is not lost
          d = -1;
          closed = fmin(closed, lb);
          ++dropped;
        } else {
          top = max(top, d - v.base + 1);
        }
      }
    }
    a.dest[ch0 + c] = d;
  }
  // 8. the state record: what stays open is the view's open slots (the parents are out) and the kept children
  double low = inf;
  int n_open = 0;
  for (int s = tid; s < in_use; s += FR_THREADS)
    if (a.p.open[v.base + s]) { low = fmin(low, a.p.bound[v.base + s]); ++n_open; }
  for (int c = c0; c < c1; ++c)
    if (a.dest[ch0 + c] >= 0) { low = fmin(low, a.ch.bound[ch0 + c]); ++n_open; }
  low = fr_block_min(red, low, tid);
  closed = fmin(v.state[FS_CLOSED_LB], fr_block_min(red, closed, tid));
  double sums[4] = {(double)n_open, (double)n_closed, (double)n_inf, (double)dropped};
  double tops = fr_block_min(red, -(double)top, tid);
  for (int q = 0; q < 4; ++q) {                         // whole numbers below 2^53: exact in any order; the tree is fixed all the same
    double w = sums[q];
    kw_block_sum<1>(red, &w, tid);
    sums[q] = w;
  }
  if (tid == 0) {
    v.state[FS_GLOBAL_UB] = gub;
    v.state[FS_CLOSED_LB] = closed;
    v.state[FS_LOWEST_OPEN] = low;
    v.state[FS_N_OPEN] = sums[0];
    v.state[FS_IN_USE] = fmax((double)in_use, -tops);
    v.state[FS_KEPT] = (double)(total_kept) - sums[3];
    v.state[FS_CLOSED] = sums[1] + sums[3];
    v.state[FS_INFEASIBLE] = sums[2];
    v.state[FS_OVERFLOW] = sums[3];
  }
}

__global__ __launch_bounds__(FR_THREADS) void k_frontier_decide(FrCommitArgs a) {
  __shared__ double red[FR_THREADS];
  __shared__ int cnt[FR_THREADS + 1];
  const FrView v{0, a.p.cap, 0, a.K, a.state, a.decision_bound};
  fr_decide(a, v, 2, red, cnt);
}

__global__ __launch_bounds__(FR_THREADS) void k_frontier_store(FrCommitArgs a) {
  const int c = blockIdx.x, d = a.dest[c];
  if (d < 0) return;
  fr_copy_row(a.s, a.p, d, a.ch, a.rmask, c);
  if (blockIdx.y == 0 && threadIdx.x == 0) {
    a.p.bound[d] = a.ch.bound[c];
    a.p.open[d] = 1;
  }
}

// ---- many jobs in one pool --------------------------------------------------------------------------------
// The pool is S segments of seg_cap slots; a segment holds one job (a box, a property row, a decision bound) and has its own record,
// so the state is (S, FS_COUNT).  A round's PLAN is one entry {segment, row0, k} per job that takes part: its k parents are rows
// [row0, row0 + k) of the batch, its children rows [2 row0, 2 row0 + 2k).  The kernels below work per entry on that segment alone:
// no reduction mixes entries, no atomic places a row, no workgroup waits on another, so an entry's result does not depend on the other
// entries, their number or their order.  gather / expand / resolve / store run unchanged: they index slots and rows globally.
//
//   * k_frontier_pick_jobs    one workgroup per entry: the k slots of lowest key among the segment's first in_use, ascending, the key
//                             being (open ? bound : +inf, slot) -- torch.sort(where(open > 0, bound, inf), stable=True)[:k].
//   * k_frontier_rows_jobs    the boxes and property rows of the n parent and 2n child rows from per-segment tables.  Plain copies.
//   * k_frontier_decide_jobs  one workgroup per entry: fr_decide on the entry's view.

struct FrPlan {
  const int32_t* plan;                                  // (n_entries, 3) {segment, row0, k}
  int n_entries, n, S, seg_cap;
};

struct FrPickArgs {
  FrPlan j; FrPool p;
  const double* state;                                  // (S, FS_COUNT)
  int32_t* slots; int32_t* row_seg;                     // (n)
};

struct FrRowsArgs {
  FrPlan j;
  int N0, NL;
  const int32_t* row_seg;
  const double* seg_x_lo; const double* seg_x_hi; const float* seg_pw; const float* seg_pb;     // (S, N_0), (S, N_L), (S)
  double* x_lo[2]; double* x_hi[2]; float* pw[2]; float* pb[2];                                  // [0]: the n parent rows, [1]: the 2n child rows
};

// an entry the host would have refused names no rows: its workgroup leaves
__device__ __forceinline__ bool fr_entry(const FrPlan& j, int e, int* seg, int* row0, int* k) {
  *seg = j.plan[3 * e]; *row0 = j.plan[3 * e + 1]; *k = j.plan[3 * e + 2];
  return *seg >= 0 && *seg < j.S && *k >= 1 && *row0 >= 0 && *row0 + *k <= j.n;
}

// (key a, slot sa) before (key b, slot sb) in torch.sort's stable ascending order: NaN after every number, equal keys by slot
__device__ __forceinline__ bool fr_key_less(double a, int sa, double b, int sb) {
  const bool an = a != a, bn = b != b;
  if (an || bn) return an == bn ? sa < sb : bn;
  return a < b || (a == b && sa < sb);
}

__global__ __launch_bounds__(FR_THREADS) void k_frontier_pick_jobs(FrPickArgs a) {
  __shared__ double rk[FR_THREADS];
  __shared__ int rs[FR_THREADS];
  const int tid = threadIdx.x;
  int seg, row0, k;
  if (!fr_entry(a.j, blockIdx.x, &seg, &row0, &k)) return;
  const double inf = __longlong_as_double(0x7ff0000000000000LL);
  const int base = seg * a.j.seg_cap;
  const int in_use = min(max((int)a.state[(long)seg * FS_COUNT + FS_IN_USE], 0), a.j.seg_cap);
  double last = 0.0;
  int last_s = -1;                                      // the slots picked so far: every (key, slot) up to (last, last_s)
  for (int r = 0; r < k; ++r) {                         // pick r: the lowest (key, slot) after the last one -- a total order, so the minimum is one slot
    double best = 0.0;
    int best_s = -1;
    for (int s = tid; s < in_use; s += FR_THREADS) {
      const double key = a.p.open[base + s] > 0 ? a.p.bound[base + s] : inf;
      if (last_s >= 0 && !fr_key_less(last, last_s, key, s)) continue;
      if (best_s < 0 || fr_key_less(key, s, best, best_s)) { best = key; best_s = s; }
    }
    rk[tid] = best; rs[tid] = best_s;
    __syncthreads();
    for (int w = FR_THREADS / 2; w > 0; w >>= 1) {
      if (tid < w) {
        const int o = rs[tid + w];
        if (o >= 0 && (rs[tid] < 0 || fr_key_less(rk[tid + w], o, rk[tid], rs[tid]))) { rk[tid] = rk[tid + w]; rs[tid] = o; }
      }
      __syncthreads();
    }
    last = rk[0]; last_s = rs[0];
    __syncthreads();
    if (last_s < 0) {                                   // fewer than k slots in use: the rows left name no slot (gather and expand skip them)
      for (int q = r + tid; q < k; q += FR_THREADS) { a.slots[row0 + q] = -1; a.row_seg[row0 + q] = seg; }
      return;
    }
    if (tid == 0) { a.slots[row0 + r] = base + last_s; a.row_seg[row0 + r] = seg; }
  }
}

__global__ __launch_bounds__(FR_THREADS) void k_frontier_rows_jobs(FrRowsArgs a) {
  const int t0 = blockIdx.y * FR_THREADS + threadIdx.x, dt = FR_SPLIT * FR_THREADS;
  const int child = (int)blockIdx.x >= a.j.n ? 1 : 0, r = (int)blockIdx.x - child * a.j.n;      // r: the row of its array
  const int seg = a.row_seg[child ? r >> 1 : r];
  if (seg < 0 || seg >= a.j.S) return;
  for (int m = t0; m < a.N0; m += dt) {
    a.x_lo[child][(long)r * a.N0 + m] = a.seg_x_lo[(long)seg * a.N0 + m];
    a.x_hi[child][(long)r * a.N0 + m] = a.seg_x_hi[(long)seg * a.N0 + m];
  }
  for (int m = t0; m < a.NL; m += dt) a.pw[child][(long)r * a.NL + m] = a.seg_pw[(long)seg * a.NL + m];
  if (t0 == 0) a.pb[child][r] = a.seg_pb[seg];
}

static_assert(sizeof(FrCommitArgs) + sizeof(FrPlan) + sizeof(double*) <= 4096, "kernel arguments: 4 KiB");

__global__ __launch_bounds__(FR_THREADS) void k_frontier_decide_jobs(FrCommitArgs a, FrPlan j, const double* decision_bound) {
  __shared__ double red[FR_THREADS];
  __shared__ int cnt[FR_THREADS + 1];
  int seg, row0, k;
  if (!fr_entry(j, blockIdx.x, &seg, &row0, &k)) return;
  const FrView v{seg * j.seg_cap, j.seg_cap, row0, k, a.state + (long)seg * FS_COUNT, decision_bound[seg]};
  fr_decide(a, v, 2, red, cnt);
}

// ---- the BaBSR fall-back below a branching threshold ---------------------------------------------------------
// Reference plnn/relu_conv_gnnkwthreshold.py:151-195 for the K parents of a round, once the GNN decisions' children (pair A) are bounded:
//
//   * k_frontier_candidates   one workgroup per parent row: the GNN's improvement of the bound (:151) and the three decisions
//                             plnn/kw_score_conv.py:115-156 can return for the row -- by score, by intercept, by layer order -- from
//                             gnnb_babsr's scores and intercepts.  Per ReLU layer the first maximum, the first minimum and the first
//                             undecided node: per-thread partials in index order, then a fixed tree on the total order (value, index),
//                             as fr_key_less is for the pick; the thread layout cannot change the result.
//   * k_frontier_fallback     one workgroup per view, ONE thread walking the view's rows in order (fr_fallback_walk): the threshold test
//                             (:155), the intercept counter's logic, the lookup of the node's inefficiency count (:160-167); writes the
//                             KW decisions, the dense list of selected parents and their number m.
//   * k_frontier_choose       one workgroup per view (fr_choose): the KW improvement (:173) and bab_caller.resolve_branching (:176-192)
//                             per selected parent, the ineff counts by one thread in row order, the final decisions.
//   * k_frontier_choose_copy  pair B's rows over pair A's, only for the parents that chose pair B; spread over workgroups as
//                             k_frontier_expand.
//
// fp32 scores are compared after promotion to double (Python's .item()); the improvement is fp64 in the reference's operation order
// (2 bound is exact, so contraction cannot change it; the division is correctly rounded).
//
// The decision rule itself -- the per-layer reduction of k_frontier_candidates and the three-way choice of fr_fallback_walk -- has this one
// text.  FrFallbackArgs.pair_a = 0 (section 7.10, at the end of this part) runs it without a pair A: every row takes part, no improvement
// is computed or tested, no inefficiency count is looked up and no selection list is written.

enum { FC_SCORE_LAY, FC_SCORE_IDX, FC_SCORE_HOLDS, FC_ICP_LAY, FC_ICP_IDX, FC_ORDER_LAY, FC_ORDER_IDX, FC_VALID, FC_COUNT };   // a row's candidates

struct FrFallbackArgs {
  FrShape s; FrPool p;
  const int32_t* slots; int K;
  const int32_t* live; const int32_t* infeasible; const double* bound;          // pair A (2K)
  const float* scores; const float* icp_tb; const float* amb;                   // (K, R)
  double branching_threshold, decision_threshold;
  int kwbd_threshold, sparsest_layer, n_order;
  int order[MAXL];
  int32_t* icp; const int32_t* ineff;
  double* gnn_imp; int32_t* kw_dec; int32_t* sel_rows; int32_t* sel_slots; int32_t* sel_dec; int32_t* m;
  int32_t* cand;                                                                // workspace (K, FC_COUNT)
  int pair_a;                                                                   // 0: BaBSR alone (section 7.10) -- no pair A, no improvement test, no selection
};

struct FrChooseArgs {
  FrShape s; FrPool p;
  int K, m;
  const int32_t* sel_rows; const int32_t* sel_slots; const int32_t* sel_dec; const int32_t* gnn_dec; const double* gnn_imp;
  FrChildren A; FrChildrenRO B;
  int32_t* ineff; double* kw_imp; int32_t* used; int32_t* dec;
};
static_assert(sizeof(FrFallbackArgs) <= 4096 && sizeof(FrChooseArgs) <= 4096, "kernel arguments: 4 KiB");

// What one job's fall-back sees of a round: its parents' rows [row0, row0 + K), the first index sel0 of its entries in the dense lists
// of selected parents, its intercept counter, its table of inefficient points, its m.  One job: {0, K, 0, icp, ineff, m}.
struct FrFbView {
  int row0, K, sel0;
  int32_t* icp; int32_t* ineff; int32_t* m;
};

__device__ __forceinline__ double fr_min0(double v) { return 0.0 < v ? 0.0 : v; }      // Python's min(v, 0)

// bab_caller.gnn_improvement (relu_conv_gnnkwthreshold.py:151), its operation order
__device__ __forceinline__ double fr_improvement(double lb0, double lb1, double bound) {
  return (fr_min0(lb0) + fr_min0(lb1) - 2.0 * bound) / (-2.0 * bound);
}

__device__ __forceinline__ double fr_child_lb(const int32_t* infeasible, const double* bound, long c) {
  return infeasible[c] ? __longlong_as_double(0x7ff0000000000000LL) : bound[c];       // an infeasible child cannot hold a counter-example
}

__device__ __forceinline__ bool fr_node(const FrShape& s, int lay, int idx, int* node) {
  if (lay < 0 || lay >= s.L || idx < 0 || idx >= s.N[lay + 1]) return false;
  *node = s.off[lay + 1] + idx;
  return true;
}

__global__ __launch_bounds__(FR_THREADS) void k_frontier_candidates(FrFallbackArgs a) {
  __shared__ float sv[FR_THREADS], mv[FR_THREADS];
  __shared__ int si[FR_THREADS], mi[FR_THREADS], ui[FR_THREADS], first[MAXL];
  const int i = blockIdx.x, tid = threadIdx.x, R = a.s.R, L = a.s.L;
  int32_t* out = a.cand + (long)i * FC_COUNT;
  const int s = a.pair_a ? a.slots[i] : 0;
  if (a.pair_a && (!fr_slot_ok(a.p, s) || !a.live[2 * i])) {      // no live GNN decision: the row takes no part (the whole workgroup leaves)
    if (tid == 0) {
      a.gnn_imp[i] = __longlong_as_double(0x7ff8000000000000LL);
      for (int q = 0; q < FC_COUNT; ++q) out[q] = q == FC_VALID || q == FC_SCORE_HOLDS ? 0 : -1;
    }
    return;
  }
  int nan = 0, any_open = 0;
  int best_l = -1, best_i = -1, icp_l = -1, icp_i = -1;
  float best_v = 0.0f;
  for (int k = 1; k <= L; ++k) {
    const int Nk = a.s.N[k];
    const long base = (long)i * R + a.s.off[k];
    float bv = 0.0f, wv = 0.0f;
    int bi = -1, wi = -1, u = -1;
    for (int j = tid; j < Nk; j += FR_THREADS) {        // index order: a strict comparison keeps the first of equal values
      const float v = a.scores[base + j], w = a.icp_tb[base + j];
      nan |= (v != v) | (w != w);
      if (bi < 0 || v > bv) { bv = v; bi = j; }
      if (wi < 0 || w < wv) { wv = w; wi = j; }
      if (u < 0 && a.amb[base + j] != 0.0f) u = j;
    }
    __syncthreads();                                    // (the previous layer's results have been read)
    sv[tid] = bv; si[tid] = bi; mv[tid] = wv; mi[tid] = wi; ui[tid] = u;
    __syncthreads();
    for (int w = FR_THREADS / 2; w > 0; w >>= 1) {      // the total orders (value, index): the first maximum, the first minimum, the first index
      if (tid < w) {
        int o = si[tid + w];
        if (o >= 0 && (si[tid] < 0 || sv[tid + w] > sv[tid] || (sv[tid + w] == sv[tid] && o < si[tid]))) { sv[tid] = sv[tid + w]; si[tid] = o; }
        o = mi[tid + w];
        if (o >= 0 && (mi[tid] < 0 || mv[tid + w] < mv[tid] || (mv[tid + w] == mv[tid] && o < mi[tid]))) { mv[tid] = mv[tid + w]; mi[tid] = o; }
        o = ui[tid + w];
        if (o >= 0 && (ui[tid] < 0 || o < ui[tid])) ui[tid] = o;
      }
      __syncthreads();
    }
    // between layers: the maximum of the tuples (value, index), the first layer that holds it; the LAST layer with an intercept below -1e-4
    if (si[0] >= 0 && (best_l < 0 || sv[0] > best_v || (sv[0] == best_v && si[0] > best_i))) { best_l = k - 1; best_i = si[0]; best_v = sv[0]; }
    if (mi[0] >= 0 && (double)mv[0] < -1e-4) { icp_l = k - 1; icp_i = mi[0]; }
    if (tid == 0) first[k - 1] = ui[0];                 // (thread 0 alone reads it back)
    any_open |= ui[0] >= 0;
  }
  nan = __syncthreads_or(nan);
  if (tid != 0) return;
  int ord_l = -1, ord_i = -1;
  for (int q = a.n_order - 1; q >= 0 && ord_l < 0; --q) {         // random_order popped from its end: the first layer with an undecided node
    const int l = a.order[q];
    if (l >= 0 && l < L && first[l] >= 0) { ord_l = l; ord_i = first[l]; }
  }
  if (a.pair_a) {
    const double bound = a.p.bound[s];
    a.gnn_imp[i] = bound < 0.0 ? fr_improvement(fr_child_lb(a.infeasible, a.bound, 2L * i), fr_child_lb(a.infeasible, a.bound, 2L * i + 1), bound) : 1.0;
  }
  out[FC_SCORE_LAY] = best_l; out[FC_SCORE_IDX] = best_i;
  out[FC_SCORE_HOLDS] = best_l >= 0 && best_l != a.sparsest_layer && (double)best_v > a.decision_threshold;
  out[FC_ICP_LAY] = icp_l; out[FC_ICP_IDX] = icp_i;
  out[FC_ORDER_LAY] = ord_l; out[FC_ORDER_IDX] = ord_i;
  out[FC_VALID] = !nan && any_open;
}

// The walk over a view's rows in order, by one thread: kw_score_conv.py:115-156 with the counter carried from row to row, then the
// selection.  The counts in ineff are read as they stood before the round (nothing here writes them).
__device__ __forceinline__ void fr_fallback_walk(const FrFallbackArgs& a, const FrFbView& v) {
  const int tid = threadIdx.x;
  for (int q = tid; q < 2 * v.K; q += blockDim.x) a.kw_dec[2L * v.row0 + q] = -1;
  __syncthreads();
  if (tid != 0) return;
  int icp = *v.icp, m = 0;
  for (int i = 0; i < v.K; ++i) {
    const int row = v.row0 + i;
    const int32_t* c = a.cand + (long)row * FC_COUNT;
    if (!c[FC_VALID] || (a.pair_a && !(a.gnn_imp[row] < a.branching_threshold))) continue;        // :155
    int lay, idx;
    if (c[FC_SCORE_HOLDS]) {
      lay = c[FC_SCORE_LAY]; idx = c[FC_SCORE_IDX];
    } else if (c[FC_ICP_LAY] >= 0 && icp < 2) {
      lay = c[FC_ICP_LAY]; idx = c[FC_ICP_IDX];
      icp = lay != 0 ? 0 : icp + 1;
    } else if (c[FC_ORDER_LAY] >= 0) {
      lay = c[FC_ORDER_LAY]; idx = c[FC_ORDER_IDX];
      icp = 0;
    } else {
      continue;                                         // random_order names no layer with an undecided node: no decision, the counter stays
    }
    a.kw_dec[2L * row] = lay; a.kw_dec[2L * row + 1] = idx;
    if (!a.pair_a) continue;                            // BaBSR alone: no table of inefficient points, no selection list
    int node;
    if (!fr_node(a.s, lay, idx, &node) || !(v.ineff[node] < a.kwbd_threshold)) continue;        // :160-167
    const int q = v.sel0 + m++;
    a.sel_rows[q] = row; a.sel_slots[q] = a.slots[row];
    a.sel_dec[2L * q] = lay; a.sel_dec[2L * q + 1] = idx;
  }
  *v.icp = icp;
  if (v.m) *v.m = m;
}

__global__ __launch_bounds__(64) void k_frontier_fallback(FrFallbackArgs a) {
  const FrFbView v{0, a.K, 0, a.icp, const_cast<int32_t*>(a.ineff), a.m};
  fr_fallback_walk(a, v);
}

// bab_caller.resolve_branching for the view's m selected parents (entries [sel0, sel0 + m) of the dense lists, pair B's rows 2q, 2q + 1).
__device__ __forceinline__ void fr_choose(const FrChooseArgs& a, const FrFbView& v, int m) {
  const int tid = threadIdx.x;
  for (int i = tid; i < v.K; i += blockDim.x) {
    const long row = v.row0 + i;
    a.dec[2 * row] = a.gnn_dec[2 * row]; a.dec[2 * row + 1] = a.gnn_dec[2 * row + 1];
    a.kw_imp[row] = -1.0;
    a.used[row] = 0;
  }
  __syncthreads();
  for (int j = tid; j < m; j += blockDim.x) {
    const long q = v.sel0 + j;
    const int row = a.sel_rows[q], s = a.sel_slots[q];
    if (row < v.row0 || row >= v.row0 + v.K || !fr_slot_ok(a.p, s) || !a.B.live[2 * q]) continue;
    const double kw = fr_improvement(fr_child_lb(a.B.infeasible, a.B.bound, 2 * q), fr_child_lb(a.B.infeasible, a.B.bound, 2 * q + 1), a.p.bound[s]);
    const double gnn = a.gnn_imp[row];
    a.kw_imp[row] = kw;
    if (kw > gnn) {                                     // :185-192 (the inefficient case, :176-184, is counted below)
      a.used[row] = 1;
      a.dec[2L * row] = a.sel_dec[2 * q]; a.dec[2L * row + 1] = a.sel_dec[2 * q + 1];
    }
  }
  __syncthreads();
  if (tid != 0) return;
  for (int j = 0; j < m; ++j) {                         // row order: two parents that name one node both count
    const long q = v.sel0 + j;
    const int row = a.sel_rows[q], s = a.sel_slots[q];
    int node;
    if (row < v.row0 || row >= v.row0 + v.K || !fr_slot_ok(a.p, s) || !a.B.live[2 * q] || !fr_node(a.s, a.sel_dec[2 * q], a.sel_dec[2 * q + 1], &node)) continue;
    const double kw = a.kw_imp[row];
    if (kw < a.gnn_imp[row] && kw < 0.05) v.ineff[node] += 1;
  }
}

__global__ __launch_bounds__(FR_THREADS) void k_frontier_choose(FrChooseArgs a) {
  const FrFbView v{0, a.K, 0, nullptr, a.ineff, nullptr};
  fr_choose(a, v, a.m);
}

__global__ __launch_bounds__(FR_THREADS) void k_frontier_choose_copy(FrChooseArgs a) {
  const int c = blockIdx.x, q = c >> 1;
  const int row = a.sel_rows[q];
  if (row < 0 || row >= a.K || !a.used[row]) return;
  const long d = 2L * row + (c & 1);
  fr_copy_row(a.s, a.A, d, a.B, a.B.mask, c);
  if (blockIdx.y == 0 && threadIdx.x == 0) {
    a.A.infeasible[d] = a.B.infeasible[c]; a.A.bound[d] = a.B.bound[c]; a.A.ubv[d] = a.B.ubv[c]; a.A.live[d] = a.B.live[c];
  }
}

// ---- the fall-back for many jobs in one pool ----------------------------------------------------------------
// The steps above per plan entry {segment, row0, k}, with the segment's intercept counter icp[segment] and its table ineff[segment]:
//
//   * k_frontier_fallback_jobs  one workgroup per entry: fr_fallback_walk on the entry's view.  The selection goes to STAGING lists at
//                               the entry's own rows ([row0, row0 + m_e)), its number to m_stage[entry]: no entry needs another's count.
//   * k_frontier_select_jobs    ONE workgroup: m_entry = {m_e per entry, M = their sum}, the exclusive prefix sum sel0 over the entries in
//                               plan order (each thread a contiguous run of entries, then a serial pass over the FR_THREADS partial sums:
//                               a fixed order for any number of entries), and entry e's staged selection to [sel0_e, sel0_e + m_e) of the
//                               dense lists.
//   * k_frontier_rows_sel       the boxes and property rows of pair B's child rows 2q, 2q + 1 (q < M) from the per-segment tables, by the
//                               segment of the selected parent's slot.  The grid covers the 2n possible rows; a workgroup with q >= M leaves.
//   * k_frontier_choose_jobs    one workgroup per entry: fr_choose on the entry's view, its dense range [sel0_e, sel0_e + m_e) from m_entry.
//
// k_frontier_candidates and k_frontier_choose_copy run unchanged on global rows (K = n).

struct FrSelArgs {
  FrPlan j;
  const int32_t* m_stage; const int32_t* st_rows; const int32_t* st_slots; const int32_t* st_dec;      // staging: (n_entries), (n), (n), (n, 2)
  int32_t* sel_rows; int32_t* sel_slots; int32_t* sel_dec; int32_t* m_entry;                           // (n), (n), (n, 2), (n_entries + 1)
  int N0, NL;
  const double* seg_x_lo; const double* seg_x_hi; const float* seg_pw; const float* seg_pb;            // (S, N_0), (S, N_L), (S)
  double* b_x_lo; double* b_x_hi; float* b_pw; float* b_pb;                                            // pair B's 2n rows
};
static_assert(sizeof(FrFallbackArgs) + sizeof(FrPlan) + sizeof(int32_t*) <= 4096 && sizeof(FrChooseArgs) + sizeof(FrPlan) + sizeof(int32_t*) <= 4096 &&
              sizeof(FrSelArgs) <= 4096, "kernel arguments: 4 KiB");

__global__ __launch_bounds__(64) void k_frontier_fallback_jobs(FrFallbackArgs a, FrPlan j, int32_t* m_stage) {
  int seg, row0, k;
  if (!fr_entry(j, blockIdx.x, &seg, &row0, &k)) return;
  const FrFbView v{row0, k, row0, a.icp + seg, const_cast<int32_t*>(a.ineff) + (long)seg * a.s.R, m_stage + blockIdx.x};
  fr_fallback_walk(a, v);
}

// m_e as the walk staged it (0 for an entry the host would have refused) and the entry's first row
__device__ __forceinline__ int fr_staged(const FrSelArgs& a, int e, int* row0) {
  int seg, k;
  if (!fr_entry(a.j, e, &seg, row0, &k)) return 0;
  return min(max(a.m_stage[e], 0), k);
}

// The compaction k_frontier_select_jobs and k_frontier_learn_compact (section 7.19) share, for ONE workgroup of FR_THREADS threads: entry e
// staged `staged(e, &row0)` items at rows [row0, row0 + that) of its staging lists; count_entry receives the counts and, last, their sum
// (at most n), and `copy(p, d)` moves staged item p to place d of the dense lists, d the exclusive prefix sum in plan order.  Each thread
// owns a contiguous run of entries; the FR_THREADS partial sums are added by one thread in a fixed order.  cnt: FR_THREADS + 1 ints of LDS.
template <class Staged, class Copy>
__device__ __forceinline__ void fr_compact_entries(int E, int n, int32_t* count_entry, int* cnt, Staged staged, Copy copy) {
  const int tid = threadIdx.x;
  const int per = (E + FR_THREADS - 1) / FR_THREADS, e0 = min(tid * per, E), e1 = min(e0 + per, E);
  int row0, sum = 0;
  for (int e = e0; e < e1; ++e) sum += staged(e, &row0);
  cnt[tid + 1] = sum;
  if (tid == 0) cnt[0] = 0;
  __syncthreads();
  if (tid == 0)
    for (int t = 1; t <= FR_THREADS; ++t) cnt[t] += cnt[t - 1];
  __syncthreads();
  int q = cnt[tid];
  for (int e = e0; e < e1; ++e) {
    const int m = staged(e, &row0);
    count_entry[e] = m;
    for (int i = 0; i < m && q + i < n; ++i) copy(row0 + i, q + i);
    q += m;
  }
  if (tid == 0) count_entry[E] = min(cnt[FR_THREADS], n);
}

__global__ __launch_bounds__(FR_THREADS) void k_frontier_select_jobs(FrSelArgs a) {
  __shared__ int cnt[FR_THREADS + 1];
  fr_compact_entries(a.j.n_entries, a.j.n, a.m_entry, cnt, [&](int e, int* row0) { return fr_staged(a, e, row0); },
                     [&](int p, int d) {
                       a.sel_rows[d] = a.st_rows[p]; a.sel_slots[d] = a.st_slots[p];
                       a.sel_dec[2L * d] = a.st_dec[2L * p]; a.sel_dec[2L * d + 1] = a.st_dec[2L * p + 1];
                     });
}

// The box and property row of segment `seg` into row c of a set of child rows: N_0 doubles twice, N_L floats, one float, over the FR_SPLIT
// workgroups of the row (blockIdx.y).  Plain copies; k_frontier_rows_sel and k_strong_rows_jobs (gnnb_k_strong.h) share it.
struct FrSegRows {
  int N0, NL;
  const double* seg_x_lo; const double* seg_x_hi; const float* seg_pw; const float* seg_pb;            // (S, N_0), (S, N_L), (S)
  double* x_lo; double* x_hi; float* pw; float* pb;                                                    // the rows
};

__device__ __forceinline__ void fr_seg_row(const FrSegRows& r, int seg, int c) {
  const int t0 = blockIdx.y * FR_THREADS + threadIdx.x, dt = FR_SPLIT * FR_THREADS;
  for (int m = t0; m < r.N0; m += dt) {
    r.x_lo[(long)c * r.N0 + m] = r.seg_x_lo[(long)seg * r.N0 + m];
    r.x_hi[(long)c * r.N0 + m] = r.seg_x_hi[(long)seg * r.N0 + m];
  }
  for (int m = t0; m < r.NL; m += dt) r.pw[(long)c * r.NL + m] = r.seg_pw[(long)seg * r.NL + m];
  if (t0 == 0) r.pb[c] = r.seg_pb[seg];
}

__global__ __launch_bounds__(FR_THREADS) void k_frontier_rows_sel(FrSelArgs a) {
  const int c = blockIdx.x, q = c >> 1;
  if (q >= a.m_entry[a.j.n_entries]) return;
  const int s = a.sel_slots[q];
  if (s < 0 || s / a.j.seg_cap >= a.j.S) return;
  const FrSegRows r{a.N0, a.NL, a.seg_x_lo, a.seg_x_hi, a.seg_pw, a.seg_pb, a.b_x_lo, a.b_x_hi, a.b_pw, a.b_pb};
  fr_seg_row(r, s / a.j.seg_cap, c);
}

__global__ __launch_bounds__(FR_THREADS) void k_frontier_choose_jobs(FrChooseArgs a, FrPlan j, const int32_t* m_entry) {
  __shared__ int red[FR_THREADS];
  const int tid = threadIdx.x, e = blockIdx.x;
  int seg, row0, k;
  if (!fr_entry(j, e, &seg, &row0, &k)) return;
  int part = 0;                                         // sel0: the m of the entries before this one (whole numbers: exact in any order)
  for (int i = tid; i < e; i += FR_THREADS) part += min(max(m_entry[i], 0), j.n);
  red[tid] = part;
  __syncthreads();
  for (int w = FR_THREADS / 2; w > 0; w >>= 1) {
    if (tid < w) red[tid] += red[tid + w];
    __syncthreads();
  }
  const int sel0 = red[0];
  const int m = min(min(max(m_entry[e], 0), k), max(a.m - sel0, 0));      // a.m: M, the host's copy of the sum
  const FrFbView v{row0, k, sel0, nullptr, a.ineff + (long)seg * a.s.R, nullptr};
  fr_choose(a, v, m);
}

// ---- BaBSR alone: relu_bab's branching -----------------------------------------------------------------------
// Reference plnn/relu_conv_any_kw.py:45-181 with split_decision = 'kw': every parent row gets the decision of kw_score_conv.py:115-156 and
// nothing else.  The rule has ONE text: k_frontier_candidates with pair_a = 0 (no slot, no pair A, no improvement: every row takes part)
// and fr_fallback_walk with pair_a = 0 (no threshold test, no table of inefficient points, no selection list), by
//
//   * k_frontier_babsr_decide        one workgroup, ONE thread walking the K rows in order with the counter *icp;
//   * k_frontier_babsr_decide_jobs   one workgroup per plan entry: the walk on the entry's rows with icp[segment].

__global__ __launch_bounds__(64) void k_frontier_babsr_decide(FrFallbackArgs a) {
  const FrFbView v{0, a.K, 0, a.icp, nullptr, nullptr};
  fr_fallback_walk(a, v);
}

__global__ __launch_bounds__(64) void k_frontier_babsr_decide_jobs(FrFallbackArgs a, FrPlan j) {
  int seg, row0, k;
  if (!fr_entry(j, blockIdx.x, &seg, &row0, &k)) return;
  const FrFbView v{row0, k, row0, a.icp + seg, nullptr, nullptr};
  fr_fallback_walk(a, v);
}

// ---- the learn rows of an online round ----------------------------------------------------------------------
// Reference plnn/relu_conv_online.py:183-207 (bab_caller.resolve_online) for the K parents of a round, once k_frontier_choose has made the
// choice: `wrong` (R) is the reference's wrong_pts_dc keyed by the flat index of the GNN's decision.
//
//   * k_frontier_learn   ONE workgroup, one thread walking the rows in order (as fr_fallback_walk does): a row that took its KW pair adds 1
//                        to wrong[flat(gnn decision)]; with the count at or above online_threshold it is a LEARN row: its row number, the
//                        flat index of its KW decision and improve = (kw_imp - gnn_imp > 0.1 ? 1 : 0), the difference in fp64, go to the
//                        dense lists in row order, n_learn their number.  Two rows that name one GNN node both count.  A row whose
//                        decisions name no node of the network is no learn row and leaves the table alone.  Entries of the lists from
//                        n_learn on are not written.

struct FrLearnArgs {
  FrShape s; int K;
  const int32_t* gnn_dec; const int32_t* kw_dec; const int32_t* used; const double* gnn_imp; const double* kw_imp;
  int online_threshold;
  int32_t* wrong; int32_t* learn_rows; int32_t* learn_kw; float* learn_imp; int32_t* n_learn;
};
static_assert(sizeof(FrLearnArgs) <= 4096, "kernel arguments: 4 KiB");

// What one job's walk sees: its rows [row0, row0 + k) of the round, the first place out0 of the lists it writes, its table and its count.
struct FrLearnView {
  int row0, k, out0;
  int32_t* wrong; int32_t* count;
};

__device__ __forceinline__ void fr_learn_walk(const FrLearnArgs& a, const FrLearnView& v) {
  if (threadIdx.x != 0) return;
  int n = 0;
  for (int i = 0; i < v.k; ++i) {
    const int row = v.row0 + i;
    if (!a.used[row]) continue;
    int gnn, kw;
    if (!fr_node(a.s, a.gnn_dec[2L * row], a.gnn_dec[2L * row + 1], &gnn) || !fr_node(a.s, a.kw_dec[2L * row], a.kw_dec[2L * row + 1], &kw)) continue;
    const int count = v.wrong[gnn] + 1;
    v.wrong[gnn] = count;
    if (count < a.online_threshold) continue;
    const int q = v.out0 + n;
    a.learn_rows[q] = row; a.learn_kw[q] = kw;
    a.learn_imp[q] = a.kw_imp[row] - a.gnn_imp[row] > 0.1 ? 1.0f : 0.0f;             // :203-206, strictly greater
    ++n;
  }
  *v.count = n;
}

__global__ __launch_bounds__(64) void k_frontier_learn(FrLearnArgs a) {
  const FrLearnView v{0, a.K, 0, a.wrong, a.n_learn};
  fr_learn_walk(a, v);
}

// ---- the learn rows of every job of a many-jobs online round ------------------------------------------------
// The walk above per plan entry {segment, row0, k}, against the segment's own table wrong[segment] (the reference builds one GraphChoice,
// and with it one wrong_pts_dc, per property):
//
//   * k_frontier_learn_jobs     one workgroup per entry, thread 0 walking the entry's rows (fr_learn_walk).  The learn rows -- GLOBAL row
//                               numbers row0 + i -- go to STAGING lists at the entry's own rows [row0, row0 + n_e), their number to
//                               n_stage[entry]: no entry needs another's count.
//   * k_frontier_learn_compact  ONE workgroup: fr_compact_entries, k_frontier_select_jobs' scheme -- learn_entry = {n_e per entry, N = their
//                               sum} and entry e's staged slice to its place in the dense lists, in plan order.  Entries of the dense
//                               lists from N on are not written.
//
// Both launch under k_frontier_learn's profile class.  In FrLearnArgs the lists are the staging lists, K is n and wrong is (S, R).

struct FrLearnSelArgs {
  FrPlan j;
  const int32_t* n_stage; const int32_t* st_rows; const int32_t* st_kw; const float* st_imp;     // staging: (n_entries), (n), (n), (n)
  int32_t* learn_rows; int32_t* learn_kw; float* learn_imp; int32_t* learn_entry;                // (n), (n), (n), (n_entries + 1)
};
static_assert(sizeof(FrLearnArgs) + sizeof(FrPlan) + sizeof(int32_t*) <= 4096 && sizeof(FrLearnSelArgs) <= 4096, "kernel arguments: 4 KiB");

__global__ __launch_bounds__(64) void k_frontier_learn_jobs(FrLearnArgs a, FrPlan j, int32_t* n_stage) {
  int seg, row0, k;
  if (!fr_entry(j, blockIdx.x, &seg, &row0, &k)) return;
  const FrLearnView v{row0, k, row0, a.wrong + (long)seg * a.s.R, n_stage + blockIdx.x};
  fr_learn_walk(a, v);
}

__global__ __launch_bounds__(FR_THREADS) void k_frontier_learn_compact(FrLearnSelArgs a) {
  __shared__ int cnt[FR_THREADS + 1];
  fr_compact_entries(a.j.n_entries, a.j.n, a.learn_entry, cnt,
                     [&](int e, int* row0) {                // n_e as the walk staged it (0 for an entry the host would have refused)
                       int seg, k;
                       if (!fr_entry(a.j, e, &seg, row0, &k)) return 0;
                       return min(max(a.n_stage[e], 0), k);
                     },
                     [&](int p, int d) { a.learn_rows[d] = a.st_rows[p]; a.learn_kw[d] = a.st_kw[p]; a.learn_imp[d] = a.st_imp[p]; });
}

// ---- the witness of the upper bound -------------------------------------------------------------------------
// Every loop of the reference returns global_ub_point next to global_ub (plnn/branch_and_bound.py:157, plnn/relu_conv_gnnkwthreshold.py:
// 209-214 and :268, plnn/relu_conv_online.py:225-228 and :276).  Between the choice and the commit, on the rows the commit will see:
//
//   * k_frontier_witness        ONE workgroup (fr_witness on the view of all K parents): the minimum of ubv over the live feasible children
//                               on the total order (value, child index) -- per-thread partials in index order, then a fixed tree, a NaN
//                               never wins, as in fr_decide -- and, when it is strictly below *best_value, that child's N_0 floats to
//                               best_point and the value to *best_value.  The point is row c of x_a, unless the parent took its KW pair
//                               (used[c >> 1]): then row 2q + (c & 1) of x_b, q the entry of the dense list with sel_rows[q] == c >> 1.
//   * k_frontier_witness_jobs   one workgroup per plan entry: fr_witness on the entry's rows, its range [sel0_e, sel0_e + m_e) of the dense
//                               lists, best_value[segment] and best_point[segment].
//
// With best_value +inf at the start, *best_value is the record's global_ub after every commit, bit for bit: both are the running fmin of
// the same values.

struct FrWitnessArgs {
  int N0;
  const int32_t* live; const int32_t* infeasible; const double* ubv;    // the children the commit will see
  const float* x_a; const float* x_b;                                   // (2n, N_0); null or pair B's
  const int32_t* used; const int32_t* sel_rows;                         // null, or as k_frontier_choose wrote them
  int K, m;
  double* best_value; float* best_point;
};
static_assert(sizeof(FrWitnessArgs) + sizeof(FrPlan) + sizeof(int32_t*) <= 4096, "kernel arguments: 4 KiB");

// What one job's witness step sees: its parents' rows [row0, row0 + K), its range [sel0, sel0 + m) of the dense lists, its incumbent.
struct FrWitView {
  int row0, K, sel0, m;
  double* best_value; float* best_point;
};

__device__ __forceinline__ void fr_witness(const FrWitnessArgs& a, const FrWitView& v, double* rv, int* ri) {
  const int tid = threadIdx.x, n = 2 * v.K;
  const long ch0 = 2L * v.row0;
  double bv = __longlong_as_double(0x7ff0000000000000LL);
  int bi = -1;
  for (int c = tid; c < n; c += FR_THREADS)             // index order: a strict comparison keeps the first of equal values, and no NaN
    if (a.live[ch0 + c] && !a.infeasible[ch0 + c]) {
      const double u = a.ubv[ch0 + c];
      if (u < bv) { bv = u; bi = c; }
    }
  rv[tid] = bv; ri[tid] = bi;
  __syncthreads();
  for (int w = FR_THREADS / 2; w > 0; w >>= 1) {        // the total order (value, index)
    if (tid < w) {
      const int o = ri[tid + w];
      if (o >= 0 && (ri[tid] < 0 || rv[tid + w] < rv[tid] || (rv[tid + w] == rv[tid] && o < ri[tid]))) { rv[tid] = rv[tid + w]; ri[tid] = o; }
    }
    __syncthreads();
  }
  const double val = rv[0], incumbent = *v.best_value;
  const int c = ri[0];
  __syncthreads();                                      // (every thread has read the incumbent before thread 0 replaces it)
  if (c < 0 || !(val < incumbent)) return;
  const long row = ch0 + c;
  const float* src = a.x_a + row * a.N0;
  if (a.used && a.used[row >> 1]) {                     // the parent took its KW pair: the value was pair B's, and so is the point
    long q = -1;
    for (int j = 0; j < v.m && q < 0; ++j)
      if (a.sel_rows[v.sel0 + j] == (int)(row >> 1)) q = v.sel0 + j;
    if (q < 0 || !a.x_b) return;                        // (lists that do not name the row: nothing is claimed)
    src = a.x_b + (2 * q + (row & 1)) * a.N0;
  }
  for (int i = tid; i < a.N0; i += FR_THREADS) v.best_point[i] = src[i];
  if (tid == 0) *v.best_value = val;
}

__global__ __launch_bounds__(FR_THREADS) void k_frontier_witness(FrWitnessArgs a) {
  __shared__ double rv[FR_THREADS];
  __shared__ int ri[FR_THREADS];
  const FrWitView v{0, a.K, 0, a.m, a.best_value, a.best_point};
  fr_witness(a, v, rv, ri);
}

__global__ __launch_bounds__(FR_THREADS) void k_frontier_witness_jobs(FrWitnessArgs a, FrPlan j, const int32_t* m_entry) {
  __shared__ double rv[FR_THREADS];
  __shared__ int ri[FR_THREADS];
  const int tid = threadIdx.x, e = blockIdx.x;
  int seg, row0, k;
  if (!fr_entry(j, e, &seg, &row0, &k)) return;
  int sel0 = 0, m = 0;
  if (a.used && m_entry) {                              // sel0 and m as k_frontier_choose_jobs has them
    int part = 0;
    for (int i = tid; i < e; i += FR_THREADS) part += min(max(m_entry[i], 0), j.n);
    ri[tid] = part;
    __syncthreads();
    for (int w = FR_THREADS / 2; w > 0; w >>= 1) {
      if (tid < w) ri[tid] += ri[tid + w];
      __syncthreads();
    }
    sel0 = ri[0];
    m = min(min(max(m_entry[e], 0), k), max(a.m - sel0, 0));
    __syncthreads();
  }
  const FrWitView v{row0, k, sel0, m, a.best_value + seg, a.best_point + (long)seg * a.N0};
  fr_witness(a, v, rv, ri);
}

// ---- several ReLUs per parent while a round is underfilled ---------------------------------------------------
// A round of K parents at DEPTH d gives every parent C = 2^d child rows, [C i, C i + C), from the candidate list gnnb_strong_list wrote
// for it (cand0 (K + 1): the exclusive prefix of the rows' counts; cand_dec (n, 2): [layer, idx] in ascending flat index).
//
//   * k_frontier_expand_depth   K parents + their lists -> C K child rows.  With m_i listed nodes, row C i + j is live for j < 2^m_i: the
//                               parent's mask with the b-th listed node set to bit b of j (0 blocked, 1 passing), split_layer the lowest
//                               layer among the nodes.  Every other row of a parent in the pool -- j >= 2^m_i, and all C rows where m_i is 0
//                               or above d, the list leaves [0, cand0[K]) or names no node of the network -- is a complete row with the
//                               parent's mask, split_layer = L - 1 and live = 0; a slot outside the pool gives k_frontier_expand's unread
//                               rows (live = 0, split_layer = -1).  fr_copy_row is the copy, the mask entries are set by the threads that
//                               copied them.  At d = 1 with the list {decisions[i]} it writes what k_frontier_expand writes.
//   * k_frontier_decide_depth   ONE workgroup: fr_decide on the view of the whole pool with C children per parent.  k_frontier_resolve and
//                               k_frontier_store run per child row as they are.

#define FR_MAX_DEPTH 8          // C <= 256 children per parent

struct FrExpandDepthArgs {
  FrShape s; FrPool p;
  const int32_t* slots; const int32_t* cand0; const int32_t* cand_dec; int K, depth;
  FrDomains ch;                                         // the K << depth children; lb / ub: gnnb_kw_bounds' parent tables
  int32_t* split; int32_t* live;
};
static_assert(sizeof(FrExpandDepthArgs) <= 4096 && sizeof(FrCommitArgs) + sizeof(int) <= 4096, "kernel arguments: 4 KiB");

__global__ __launch_bounds__(FR_THREADS) void k_frontier_expand_depth(FrExpandDepthArgs a) {
  const int c = blockIdx.x, i = c >> a.depth, j = c & ((1 << a.depth) - 1), t0 = blockIdx.y * FR_THREADS + threadIdx.x, dt = FR_SPLIT * FR_THREADS;
  const int s = a.slots[i];
  if (!fr_slot_ok(a.p, s)) {                            // no such parent: a dead row nobody reads
    if (t0 == 0) { a.live[c] = 0; a.split[c] = -1; }
    return;
  }
  const int q0 = a.cand0[i], m = a.cand0[i + 1] - q0;
  bool listed = q0 >= 0 && m >= 1 && m <= a.depth && q0 + m <= a.cand0[a.K];
  int node[FR_MAX_DEPTH], lay = a.s.L;
#pragma unroll
  for (int b = 0; b < FR_MAX_DEPTH; ++b) {              // (unrolled: node[] stays in registers)
    node[b] = -1;
    if (listed && b < m) {
      const int l = a.cand_dec[2L * (q0 + b)];
      if (fr_node(a.s, l, a.cand_dec[2L * (q0 + b) + 1], &node[b])) lay = min(lay, l);
      else listed = false;
    }
  }
  const bool live = listed && j < (1 << m);
  fr_copy_row(a.s, a.ch, c, a.p, a.p.mask, s);
  if (live) {
#pragma unroll
    for (int b = 0; b < FR_MAX_DEPTH; ++b)              // by the thread that copied the entry: no second pass
      if (b < m && node[b] % dt == t0) a.ch.mask[(long)c * a.s.R + node[b]] = (int8_t)((j >> b) & 1);
  }
  if (t0 == 0) {
    a.live[c] = live ? 1 : 0;
    a.split[c] = live ? lay : a.s.L - 1;                // a dead row keeps every bound of its parent
  }
}

__global__ __launch_bounds__(FR_THREADS) void k_frontier_decide_depth(FrCommitArgs a, int depth) {
  __shared__ double red[FR_THREADS];
  __shared__ int cnt[FR_THREADS + 1];
  const FrView v{0, a.p.cap, 0, a.K, a.state, a.decision_bound};
  fr_decide(a, v, 1 << depth, red, cnt);
}
