// gnnb_k_starts.h -- the upper bound from many starts: the restarts of the reference's get_upper_bound_pgd
// (plnn/conv_kwinter_gen.py:54-135: the LP point in slot 0, uniform points of the domain in the others) and of its sibling
// get_upper_bound_random (:20-52), on the device.
//
//   * k_net_starts          the start points of B rows: slot 0 = x0[b], slot r >= 1 a counter-based uniform point of the row's box.  No
//                           generator state: coordinate (r, m) of a row is a hash of the row's KEY and its own counter, and the key is
//                           seed + an integer sum over the row's x0 -- so a row's starts depend on its own x0, box and seed only, never on
//                           B, its index or what ran before.
//   * k_net_descend_tile<S> one workgroup carries S starts of ONE row through every layer together: k_net_descend's rule per start, with
//                           the activations and gradients laid out [node][S].  Each weight, each tap's index arithmetic and each gate
//                           address is computed once and feeds S independent accumulators; a Linear row's butterfly runs S times over
//                           the same lanes; the layer barriers are paid once per S starts.  Every start's sums are k_net_descend's sums
//                           in k_net_descend's order.  A start that has stopped is masked: its point is frozen, its accumulators still run
//                           (nobody reads them).  A tile ends when all its starts have stopped, or after n_steps.  A start with a NaN
//                           coordinate takes no step and its value IS a NaN (fmax in a ReLU would swallow it, and what is left is the
//                           network's value at no point of the box): it never wins the pick.
//   * k_net_starts_pick     one workgroup per row: the minimum of the starts' best values in the total order (value, start index),
//                           strict <, a NaN never wins, all NaN -> start 0; the winner's point and value go to x_best / value.
//
// No atomics, no workgroup waits on another, every sum in a fixed order.

#define NS_TILE 4               // S: starts one workgroup of k_net_descend_tile carries
#define NS_SLOTS 16             // start slots one workgroup of k_net_starts fills
#define NS_MAX_RANDOM 4096      // R, the random starts of a row: 0..NS_MAX_RANDOM

#define NS_GOLDEN 0x9E3779B97F4A7C15ull

// the splitmix64 finaliser
__host__ __device__ __forceinline__ unsigned long long ns_mix(unsigned long long z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

struct NetStartsArgs {
  const float* x0; const double* x_lo; const double* x_hi;      // (B, N_0) x 3
  float* starts;                                                // (B, R + 1, N_0)
  int N0, R;
  unsigned long long seed;
};

__global__ __launch_bounds__(FR_THREADS) void k_net_starts(NetStartsArgs a) {
  __shared__ unsigned long long part[FR_THREADS];
  const int b = blockIdx.x, tid = threadIdx.x, N0 = a.N0;
  const float* x0 = a.x0 + (long)b * N0;
  const double* lo = a.x_lo + (long)b * N0;
  const double* hi = a.x_hi + (long)b * N0;
  const int r0 = blockIdx.y * NS_SLOTS, r1 = min(r0 + NS_SLOTS, a.R + 1);
  float* out = a.starts + (long)b * (a.R + 1) * N0;
  // the row's key: an integer sum (mod 2^64), the same in any order
  unsigned long long k = 0;
  for (int m = tid; m < N0; m += FR_THREADS) k += ns_mix((unsigned long long)__float_as_uint(x0[m]) + ((unsigned long long)m << 32));
  part[tid] = k;
  __syncthreads();
  for (int s = FR_THREADS / 2; s > 0; s >>= 1) {
    if (tid < s) part[tid] += part[tid + s];
    __syncthreads();
  }
  const unsigned long long key = a.seed + part[0];
  for (int r = r0; r < r1; ++r) {
    float* row = out + (long)r * N0;
    if (r == 0) {
      for (int m = tid; m < N0; m += FR_THREADS) row[m] = x0[m];
      continue;
    }
    for (int m = tid; m < N0; m += FR_THREADS) {
      const unsigned long long c = (unsigned long long)r * (unsigned long long)N0 + (unsigned long long)m + 1ull;
      const double u = (double)(ns_mix(key + NS_GOLDEN * c) >> 11) * 0x1.0p-53;
      const double l = lo[m], h = hi[m], v = fma(h - l, u, l);
      float f = (float)v;                               // to nearest; where that leaves [l, h], the neighbouring float inside
      if ((double)f < l) f = nextafterf(f, __builtin_inff());
      else if ((double)f > h) f = nextafterf(f, -__builtin_inff());
      row[m] = f;
    }
  }
}

// ---- S starts of one row through the network together --------------------------------------------------------------------------------
struct NetTileArgs {
  KwNet net;
  const float* starts; int n_starts;                    // (B, n_starts, N_0)
  const double* x_lo; const double* x_hi; const float* prop_w; const float* prop_b;     // (B, N_0) x 2, (B, N_L), (B)
  int n_steps; double step;
  float* xb; double* val; int32_t* steps_taken;         // per start: (B, n_starts, N_0), (B, n_starts), null or (B, n_starts)
  double* ws; long ws_stride;                           // per tile: S x (the activations of graph layers 0..L, then two gradient buffers of `width`), [node][S]
  int act_off[MAXL + 2], width;
};
static_assert(sizeof(NetTileArgs) <= 4096, "kernel arguments: 4 KiB");

struct NetPickArgs {
  const float* xb; const double* val;                   // (B, n_starts, N_0), (B, n_starts)
  int n_starts, N0;
  float* x_best; double* value; int32_t* start_index; double* start_value;      // (B, N_0), (B), null or (B), null or (B, n_starts)
};

// dual_conv_at for S columns of q laid out [node][S]: the taps in dual_conv_at's order
template <int S>
__device__ __forceinline__ void tile_conv_at(const KwEdge& E, int j, const double* q, double (&acc)[S]) {
  const int hw = E.h_out * E.w_out, co = j / hw, oy = (j % hw) / E.w_out, ox = j % E.w_out;
  const double* w = E.w + (long)co * E.c_in * E.kh * E.kw;
#pragma unroll
  for (int s = 0; s < S; ++s) acc[s] = 0.0;
  for (int ci = 0; ci < E.c_in; ++ci)
    for (int ky = 0; ky < E.kh; ++ky) {
      const int iy = oy * E.stride - E.pad + ky;
      if (iy < 0 || iy >= E.h_in) continue;
      for (int kx = 0; kx < E.kw; ++kx) {
        const int ix = ox * E.stride - E.pad + kx;
        if (ix < 0 || ix >= E.w_in) continue;
        const double c = w[(ci * E.kh + ky) * E.kw + kx];
        const double* qp = q + (((long)ci * E.h_in + iy) * E.w_in + ix) * S;
#pragma unroll
        for (int s = 0; s < S; ++s) acc[s] += c * qp[s];
      }
    }
}

// kw_transpose_at over the whole output for S columns of nu laid out [node][S]: the taps in kw_transpose_at's order
template <int S>
__device__ __forceinline__ void tile_transpose_at(const KwEdge& E, int m, const double* nu, double (&acc)[S]) {
  const double* w = E.w;
#pragma unroll
  for (int s = 0; s < S; ++s) acc[s] = 0.0;
  if (E.kind == 1) {
    for (int o = 0; o < E.n_out; ++o) {
      const double c = w[(long)o * E.n_in + m];
#pragma unroll
      for (int s = 0; s < S; ++s) acc[s] += c * nu[(long)o * S + s];
    }
    return;
  }
  const int hwi = E.h_in * E.w_in, ci = m / hwi, iy = (m % hwi) / E.w_in, ix = m % E.w_in;
  const int ntap = E.c_in * E.kh * E.kw;
  for (int ky = 0; ky < E.kh; ++ky) {
    const int ty = iy + E.pad - ky;
    if (ty < 0 || ty % E.stride) continue;
    const int oy = ty / E.stride;
    if (oy > E.h_out - 1) continue;
    for (int kx = 0; kx < E.kw; ++kx) {
      const int tx = ix + E.pad - kx;
      if (tx < 0 || tx % E.stride) continue;
      const int ox = tx / E.stride;
      if (ox > E.w_out - 1) continue;
      const double* wp = w + ((long)ci * E.kh + ky) * E.kw + kx;
      const double* np = nu + ((long)oy * E.w_out + ox) * S;
      for (int co = 0; co < E.c_out; ++co) {
        const double c = wp[(long)co * ntap];
        const double* nq = np + (long)co * E.h_out * E.w_out * S;
#pragma unroll
        for (int s = 0; s < S; ++s) acc[s] += c * nq[s];
      }
    }
  }
}

// net_forward for S points: at(k) is where graph layer k's activations live, [node][S]; f[s] on every thread.  red: S * FR_THREADS doubles
template <int S, class At>
__device__ __forceinline__ void net_forward_tile(const KwNet& net, const float* prop_w, float prop_b, At at, double* red, int tid, double (&f)[S]) {
  const int lane = tid & 63, wave = tid >> 6;
  for (int k = 1; k <= net.L; ++k) {
    const KwEdge& E = net.e[k];
    const int Nk = net.N[k];
    const double* cur = at(k - 1);
    double* nxt = at(k);
    if (E.kind == 0) {
      const int hw = E.h_out * E.w_out;
      for (int j = tid; j < Nk; j += FR_THREADS) {
        double acc[S];
        tile_conv_at<S>(E, j, cur, acc);
        const double bias = E.bias[j / hw];
#pragma unroll
        for (int s = 0; s < S; ++s) nxt[(long)j * S + s] = fmax(acc[s] + bias, 0.0);
      }
    } else {
      for (int j = wave; j < Nk; j += FR_THREADS / 64) {
        const double* row = E.w + (long)j * E.n_in;
        double acc[S];
#pragma unroll
        for (int s = 0; s < S; ++s) acc[s] = 0.0;
        for (int t = lane; t < E.n_in; t += 64) {
          const double c = row[t];
#pragma unroll
          for (int s = 0; s < S; ++s) acc[s] += c * cur[(long)t * S + s];
        }
#pragma unroll
        for (int s = 0; s < S; ++s)
          for (int d = 32; d > 0; d >>= 1) acc[s] += __shfl_xor(acc[s], d, 64);
        if (lane == 0) {
          const double bias = E.bias[j];
#pragma unroll
          for (int s = 0; s < S; ++s) nxt[(long)j * S + s] = fmax(acc[s] + bias, 0.0);
        }
      }
    }
    __syncthreads();
  }
  const int NL = net.N[net.L];
  const double* cur = at(net.L);
#pragma unroll
  for (int s = 0; s < S; ++s) f[s] = 0.0;
  for (int j = tid; j < NL; j += FR_THREADS) {
    const double c = (double)prop_w[j];
#pragma unroll
    for (int s = 0; s < S; ++s) f[s] += c * cur[(long)j * S + s];
  }
  kw_block_sum<S>(red, f, tid);
#pragma unroll
  for (int s = 0; s < S; ++s) f[s] = f[s] + (double)prop_b;
}

// net_backward for S points: returns the buffer (ga or gb) that holds the N_0 x S entries, synchronised
template <int S>
__device__ __forceinline__ double* net_backward_tile(const NetTileArgs& a, const double* act, const float* prop_w, double* ga, double* gb, int tid) {
  const KwNet& net = a.net;
  const double* top = act + (long)a.act_off[net.L] * S;
  for (int j = tid; j < net.N[net.L]; j += FR_THREADS) {
    const double c = (double)prop_w[j];
#pragma unroll
    for (int s = 0; s < S; ++s) ga[(long)j * S + s] = top[(long)j * S + s] > 0.0 ? c : 0.0;
  }
  __syncthreads();
  double* cur = ga;
  double* nxt = gb;
  for (int k = net.L; k >= 1; --k) {
    const KwEdge& E = net.e[k];
    const double* below = act + (long)a.act_off[k - 1] * S;
    for (int m = tid; m < net.N[k - 1]; m += FR_THREADS) {      // (a gated node is exactly 0; the input layer has no gate)
      bool open[S], any = false;
#pragma unroll
      for (int s = 0; s < S; ++s) { open[s] = k == 1 || below[(long)m * S + s] > 0.0; any |= open[s]; }
      double acc[S];
      if (any) tile_transpose_at<S>(E, m, cur, acc);
#pragma unroll
      for (int s = 0; s < S; ++s) nxt[(long)m * S + s] = open[s] ? acc[s] : 0.0;
    }
    double* t = cur; cur = nxt; nxt = t;
    __syncthreads();
  }
  return cur;
}

template <int S>
__global__ __launch_bounds__(FR_THREADS) void k_net_descend_tile(NetTileArgs a) {
  __shared__ double red[S * FR_THREADS];
  const int tiles = (a.n_starts + S - 1) / S;
  const int b = blockIdx.x / tiles, s0 = (blockIdx.x % tiles) * S, tid = threadIdx.x;
  const int ns = min(S, a.n_starts - s0);               // the last tile of a row may be partly empty: its empty columns carry a copy of column 0, masked
  const KwNet& net = a.net;
  const int N0 = net.N[0];
  double* act = a.ws + (long)blockIdx.x * a.ws_stride;
  double* ga = act + (long)a.act_off[net.L + 1] * S;
  double* gb = ga + (long)a.width * S;
  const float* x0 = a.starts + ((long)b * a.n_starts + s0) * N0;
  float* xb = a.xb + ((long)b * a.n_starts + s0) * N0;
  const double* lo = a.x_lo + (long)b * N0;
  const double* hi = a.x_hi + (long)b * N0;
  const float* pw = a.prop_w + (long)b * net.N[net.L];
  const float pb = a.prop_b[b];
  const auto at = [&](int k) { return act + (long)a.act_off[k] * S; };
  int nanm = 0;
  for (int m = tid; m < N0; m += FR_THREADS) {
#pragma unroll
    for (int s = 0; s < S; ++s) {
      const float v = x0[(long)(s < ns ? s : 0) * N0 + m];
      if (s < ns) xb[(long)s * N0 + m] = v;             // best = (f(x0), x0), unconditionally
      act[(long)m * S + s] = (double)v;
      nanm |= (v != v) << s;
    }
  }
  bool on[S], nan[S];                                   // the starts still descending; those with a NaN coordinate (the same on all threads)
#pragma unroll
  for (int s = 0; s < S; ++s) { nan[s] = __syncthreads_or(nanm >> s & 1); on[s] = !nan[s]; }
  double f[S], best[S], fn[S];
  int steps[S];
  net_forward_tile<S>(net, pw, pb, at, red, tid, f);
  bool any = false;
#pragma unroll
  for (int s = 0; s < S; ++s) {
    best[s] = f[s];
    steps[s] = 0;
    on[s] = on[s] && s < ns && a.n_steps > 0 && f[s] == f[s];
    any |= on[s];
  }
  const double* g = nullptr;
  if (any) g = net_backward_tile<S>(a, act, pw, ga, gb, tid);
  for (int t = 0; any && t < a.n_steps; ++t) {
    for (int m = tid; m < N0; m += FR_THREADS) {
      const double l = lo[m], h = hi[m];
#pragma unroll
      for (int s = 0; s < S; ++s) {
        if (!on[s]) continue;                           // a stopped start's point is frozen
        const double x = act[(long)m * S + s], d = a.step * (h - l), gm = g[(long)m * S + s];
        double v = gm > 0.0 ? x - d : (gm < 0.0 ? x + d : x);
        v = fmin(fmax(v, l), h);
        float r = (float)v;                             // to nearest; where that leaves [l, h], the neighbouring float inside
        if ((double)r < l) r = nextafterf(r, __builtin_inff());
        else if ((double)r > h) r = nextafterf(r, -__builtin_inff());
        act[(long)m * S + s] = (double)r;
      }
    }
    __syncthreads();
    net_forward_tile<S>(net, pw, pb, at, red, tid, fn);
    any = false;
#pragma unroll
    for (int s = 0; s < S; ++s) {
      if (!on[s]) continue;
      ++steps[s];
      if (fn[s] < best[s]) {
        best[s] = fn[s];
        for (int m = tid; m < N0; m += FR_THREADS) xb[(long)s * N0 + m] = (float)act[(long)m * S + s];
      }
      if (!(fn[s] < f[s])) on[s] = false;               // the reference's stop rule; a NaN stops here too
      else f[s] = fn[s];
      any |= on[s];
    }
    if (any && t + 1 < a.n_steps) g = net_backward_tile<S>(a, act, pw, ga, gb, tid);
  }
  if (tid == 0) {
#pragma unroll
    for (int s = 0; s < S; ++s) {
      if (s >= ns) continue;
      a.val[(long)b * a.n_starts + s0 + s] = nan[s] ? __builtin_nan("") : best[s];      // (a ReLU's fmax swallows a NaN: the value left is no upper bound)
      if (a.steps_taken) a.steps_taken[(long)b * a.n_starts + s0 + s] = steps[s];
    }
  }
}

// the better of two candidates in the total order (value, start index); index -1: none yet (a NaN is never a candidate)
__device__ __forceinline__ void ns_better(double& v, int& i, double w, int j) {
  if (j >= 0 && (i < 0 || w < v || (w == v && j < i))) { v = w; i = j; }
}

__global__ __launch_bounds__(FR_THREADS) void k_net_starts_pick(NetPickArgs a) {
  __shared__ double sv[FR_THREADS];
  __shared__ int si[FR_THREADS];
  const int b = blockIdx.x, tid = threadIdx.x, n = a.n_starts;
  const double* val = a.val + (long)b * n;
  double v = 0.0;
  int i = -1;
  for (int r = tid; r < n; r += FR_THREADS) {
    const double w = val[r];
    if (a.start_value) a.start_value[(long)b * n + r] = w;
    ns_better(v, i, w, w == w ? r : -1);
  }
  sv[tid] = v; si[tid] = i;
  __syncthreads();
  for (int s = FR_THREADS / 2; s > 0; s >>= 1) {
    if (tid < s) {
      double v0 = sv[tid]; int i0 = si[tid];
      ns_better(v0, i0, sv[tid + s], si[tid + s]);
      sv[tid] = v0; si[tid] = i0;
    }
    __syncthreads();
  }
  const int win = si[0] < 0 ? 0 : si[0];                // every value a NaN: start 0 and its NaN
  const float* src = a.xb + ((long)b * n + win) * a.N0;
  for (int m = tid; m < a.N0; m += FR_THREADS) a.x_best[(long)b * a.N0 + m] = src[m];
  if (tid == 0) {
    a.value[b] = val[win];
    if (a.start_index) a.start_index[b] = win;
  }
}
