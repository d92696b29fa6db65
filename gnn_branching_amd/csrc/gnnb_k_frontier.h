// gnnb_k_frontier.h -- the per-round steps of a branch-and-bound loop whose open domains stay in device memory:
// gnnb_frontier_gather, gnnb_frontier_expand, gnnb_net_eval, gnnb_frontier_commit.  Between them run the existing batch kernels
// (gnnb_dual_ascent at n_iter = 0 for the scorer's inputs, gnnb_forward, gnnb_kw_bounds, gnnb_dual_ascent), untouched.
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
//   * k_net_eval          the bound network + a property row at B points in fp64: one workgroup per point, activations in the
//                         workspace (two buffers of the widest graph layer), a conv node per thread (dual_conv_at), a Linear row per
//                         wave with the fixed butterfly -- the shapes of dual_forward.
//   * k_frontier_resolve  per child: the mask resolved by the bounds (-1 with lo >= 0 -> 1, -1 with up <= 0 -> 0) and whether an
//                         undecided node is left.
//   * k_frontier_decide   ONE workgroup: global_ub, keep or close every child, the parents' slots freed, the kept children's
//                         destination slots by a prefix sum over the 2K keep flags in child order, the state record.
//   * k_frontier_store    kept children -> their pool slots.
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

struct FrPool {
  int8_t* mask; double* lb[MAXL + 2]; double* ub[MAXL + 2];     // lb / ub: graph layers 1..L+1
  double* alpha; double* beta; double* bound; int32_t* open;
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
  int8_t* mask; double* plb[MAXL + 2]; double* pub[MAXL + 2];
  int32_t* split; double* alpha; double* beta; int32_t* live;
};

struct FrCommitArgs {
  FrShape s; FrPool p;
  const int32_t* slots; int K;
  const int8_t* mask; const double* lb[MAXL + 2]; const double* ub[MAXL + 2];    // the 2K children
  const int32_t* infeasible; const double* bound; const double* alpha; const double* beta; const double* ubv; const int32_t* live;
  double eps, decision_bound;
  double* state;
  int8_t* rmask; int32_t* undecided; int32_t* dest;     // workspace: (2K, R), (2K), (2K)
};
static_assert(sizeof(FrGatherArgs) <= 4096 && sizeof(FrExpandArgs) <= 4096 && sizeof(FrCommitArgs) <= 4096, "kernel arguments: 4 KiB");

__device__ __forceinline__ bool fr_slot_ok(const FrPool& p, int s) { return s >= 0 && s < p.cap; }

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
  const int R = a.s.R, K1 = a.s.L + 1;
  const int lay = a.decisions[2 * i], idx = a.decisions[2 * i + 1];
  const bool live = lay >= 0 && lay < a.s.L && idx >= 0 && idx < a.s.N[lay + 1];
  const int node = live ? a.s.off[lay + 1] + idx : -1;
  for (int r = t0; r < R; r += dt) {
    a.mask[(long)c * R + r] = r == node ? (int8_t)choice : a.p.mask[(long)s * R + r];
    a.alpha[(long)c * R + r] = a.p.alpha[(long)s * R + r];
    a.beta[(long)c * R + r] = a.p.beta[(long)s * R + r];
  }
  for (int k = 1; k <= K1; ++k) {
    const int Nk = a.s.N[k];
    for (int j = t0; j < Nk; j += dt) {
      a.plb[k][(long)c * Nk + j] = a.p.lb[k][(long)s * Nk + j];
      a.pub[k][(long)c * Nk + j] = a.p.ub[k][(long)s * Nk + j];
    }
  }
  if (t0 == 0) {
    a.live[c] = live ? 1 : 0;
    a.split[c] = live ? lay : a.s.L - 1;                // a dead row keeps every bound of its parent
  }
}

struct NetEvalArgs {
  KwNet net;
  const float* x; const float* prop_w; const float* prop_b;     // (B, N_0), (B, N_L), (B)
  double* out;                                                  // (B)
  double* ws; long ws_stride;                                   // 2 * widest graph layer doubles per point
};

static inline int net_eval_width(const KwNet& n) {
  int w = 1;
  for (int k = 0; k <= n.L; ++k) w = n.N[k] > w ? n.N[k] : w;
  return w;
}

__global__ __launch_bounds__(FR_THREADS) void k_net_eval(NetEvalArgs a) {
  __shared__ double red[FR_THREADS];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  double* cur = a.ws + (long)b * a.ws_stride;
  double* nxt = cur + a.ws_stride / 2;
  const int N0 = a.net.N[0];
  for (int m = tid; m < N0; m += FR_THREADS) cur[m] = (double)a.x[(long)b * N0 + m];
  __syncthreads();
  for (int k = 1; k <= a.net.L; ++k) {
    const KwEdge& E = a.net.e[k];
    const int Nk = a.net.N[k];
    if (E.kind == 0) {
      const int hw = E.h_out * E.w_out;
      for (int j = tid; j < Nk; j += FR_THREADS) nxt[j] = fmax(dual_conv_at(E, j, cur) + E.bias[j / hw], 0.0);
    } else {
      for (int j = wave; j < Nk; j += FR_THREADS / 64) {
        const double* row = E.w + (long)j * E.n_in;
        double acc = 0.0;
        for (int t = lane; t < E.n_in; t += 64) acc += row[t] * cur[t];
        for (int s = 32; s > 0; s >>= 1) acc += __shfl_xor(acc, s, 64);
        if (lane == 0) nxt[j] = fmax(acc + E.bias[j], 0.0);
      }
    }
    double* t = cur; cur = nxt; nxt = t;
    __syncthreads();
  }
  const int NL = a.net.N[a.net.L];
  double part = 0.0;
  for (int j = tid; j < NL; j += FR_THREADS) part += (double)a.prop_w[(long)b * NL + j] * cur[j];
  kw_block_sum<1>(red, &part, tid);
  if (tid == 0) a.out[b] = part + (double)a.prop_b[b];
}

__global__ __launch_bounds__(FR_THREADS) void k_frontier_resolve(FrCommitArgs a) {
  const int c = blockIdx.x, tid = threadIdx.x, R = a.s.R;
  int open = 0;
  if (a.live[c]) {                                      // (a dead row's arrays are never read)
    for (int k = 1; k <= a.s.L; ++k) {
      const int Nk = a.s.N[k];
      for (int j = tid; j < Nk; j += FR_THREADS) {
        const long r = (long)c * R + a.s.off[k] + j;
        int m = a.mask[r];
        if (m == -1 && a.lb[k][(long)c * Nk + j] >= 0.0) m = 1;
        if (m == -1 && a.ub[k][(long)c * Nk + j] <= 0.0) m = 0;
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

__global__ __launch_bounds__(FR_THREADS) void k_frontier_decide(FrCommitArgs a) {
  __shared__ double red[FR_THREADS];
  __shared__ int cnt[FR_THREADS + 1];
  const int tid = threadIdx.x, K = a.K, n = 2 * K;
  const double inf = __longlong_as_double(0x7ff0000000000000LL);
  const int in_use = min(max((int)a.state[FS_IN_USE], 0), a.p.cap);
  // 2. the incumbent: every live feasible child's network value at its LP point
  double v = inf;
  for (int c = tid; c < n; c += FR_THREADS)
    if (a.live[c] && !a.infeasible[c]) v = fmin(v, a.ubv[c]);
  const double gub = fmin(a.state[FS_GLOBAL_UB], fr_block_min(red, v, tid));
  // 3. - 5. keep or close (each thread a contiguous run of children, so that ranks follow child order)
  const int per = (n + FR_THREADS - 1) / FR_THREADS, c0 = min(tid * per, n), c1 = min(c0 + per, n);
  const bool have_db = a.decision_bound == a.decision_bound;
  double closed = inf;
  int kept = 0, n_closed = 0, n_inf = 0;
  for (int c = c0; c < c1; ++c) {
    if (!a.live[c]) continue;
    if (a.infeasible[c]) { ++n_inf; continue; }
    const double lb = a.bound[c];
    if (a.undecided[c] && lb < gub - a.eps && (!have_db || lb < a.decision_bound)) ++kept;
    else { closed = fmin(closed, lb); ++n_closed; }
  }
  for (int i = tid; i < K; i += FR_THREADS) {           // a parent without a live child (decision [-1, -1]) is closed at its own bound
    const int s = a.slots[i];
    if (fr_slot_ok(a.p, s) && !a.live[2 * i] && !a.live[2 * i + 1]) { closed = fmin(closed, a.p.bound[s]); ++n_closed; }
  }
  // 6. the parents leave the pool
  for (int i = tid; i < K; i += FR_THREADS)
    if (fr_slot_ok(a.p, a.slots[i])) a.p.open[a.slots[i]] = 0;
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
    if (a.live[c] && !a.infeasible[c]) {
      const double lb = a.bound[c];
      if (a.undecided[c] && lb < gub - a.eps && (!have_db || lb < a.decision_bound)) {
        d = rank < K ? a.slots[rank] : in_use + (rank - K);
        ++rank;
        if (!fr_slot_ok(a.p, d)) {                      // no room (the caller checks the capacity before a round): the bound is not lost
          d = -1;
          closed = fmin(closed, lb);
          ++dropped;
        } else {
          top = max(top, d + 1);
        }
      }
    }
    a.dest[c] = d;
  }
  // 8. the state record: what stays open is the pool's open slots (the parents are out) and the kept children
  double low = inf;
  int n_open = 0;
  for (int s = tid; s < in_use; s += FR_THREADS)
    if (a.p.open[s]) { low = fmin(low, a.p.bound[s]); ++n_open; }
  for (int c = c0; c < c1; ++c)
    if (a.dest[c] >= 0) { low = fmin(low, a.bound[c]); ++n_open; }
  low = fr_block_min(red, low, tid);
  closed = fmin(a.state[FS_CLOSED_LB], fr_block_min(red, closed, tid));
  double sums[4] = {(double)n_open, (double)n_closed, (double)n_inf, (double)dropped};
  double tops = fr_block_min(red, -(double)top, tid);
  for (int q = 0; q < 4; ++q) {                         // whole numbers below 2^53: exact in any order; the tree is fixed all the same
    double w = sums[q];
    kw_block_sum<1>(red, &w, tid);
    sums[q] = w;
  }
  if (tid == 0) {
    a.state[FS_GLOBAL_UB] = gub;
    a.state[FS_CLOSED_LB] = closed;
    a.state[FS_LOWEST_OPEN] = low;
    a.state[FS_N_OPEN] = sums[0];
    a.state[FS_IN_USE] = fmax((double)in_use, -tops);
    a.state[FS_KEPT] = (double)(total_kept) - sums[3];
    a.state[FS_CLOSED] = sums[1] + sums[3];
    a.state[FS_INFEASIBLE] = sums[2];
    a.state[FS_OVERFLOW] = sums[3];
  }
}

__global__ __launch_bounds__(FR_THREADS) void k_frontier_store(FrCommitArgs a) {
  const int c = blockIdx.x, t0 = blockIdx.y * FR_THREADS + threadIdx.x, dt = FR_SPLIT * FR_THREADS;
  const int d = a.dest[c];
  if (d < 0) return;
  const int R = a.s.R, K1 = a.s.L + 1;
  for (int r = t0; r < R; r += dt) {
    a.p.mask[(long)d * R + r] = a.rmask[(long)c * R + r];
    a.p.alpha[(long)d * R + r] = a.alpha[(long)c * R + r];
    a.p.beta[(long)d * R + r] = a.beta[(long)c * R + r];
  }
  for (int k = 1; k <= K1; ++k) {
    const int Nk = a.s.N[k];
    for (int j = t0; j < Nk; j += dt) {
      a.p.lb[k][(long)d * Nk + j] = a.lb[k][(long)c * Nk + j];
      a.p.ub[k][(long)d * Nk + j] = a.ub[k][(long)c * Nk + j];
    }
  }
  if (t0 == 0) {
    a.p.bound[d] = a.bound[c];
    a.p.open[d] = 1;
  }
}
