// gnnb_k_net.h -- the fp64 walk of the bound network: forward through every layer, backward through the gates, and the projected
// signed-gradient descent built on the two (DESIGN.md sections 7.8 and 7.9; reference plnn/conv_kwinter_gen.py:54-135, get_upper_bound_pgd,
// called from each child's LP point by plnn/relu_conv_any_kw.py:143-149).  ONE text, templated on S, the points a workgroup carries
// together, laid out [node][S]: each weight, each tap's index arithmetic and each gate address is computed once and feeds S independent
// accumulators; a Linear row's butterfly runs S times over the same lanes; the layer barriers are paid once per S points.  A point's sums
// and their order do not depend on S or on its column: at S = 1 the [S] arrays are scalars.  The kernels are wrappers:
//
//   * k_net_eval            S = 1.  The bound network + a property row at B points: one workgroup per point, activations in two
//                           ping-pong buffers of the widest graph layer (its at(k)), a conv node per thread, a Linear row per wave with
//                           the fixed butterfly -- the shapes of dual_forward.
//   * k_net_descend         S = 1, NET_POINTS.  One workgroup per point, the activations of EVERY graph layer 0..L kept in the workspace.
//   * k_net_descend_tile<S> NET_STARTS.  One workgroup carries S starts of ONE row; the last tile of a row may be partly empty.
//
// The descent: f is net_forward; g the backward pass through its activations: g_L = prop_w . 1[act_L > 0], down each edge by its
// transpose (a conv's taps in a fixed order, a Linear map's column), gated by 1[act_k > 0] at every ReLU layer (torch's ReLU gradient).
// best = (f(x0), x0); then up to n_steps times
//   x'[m] = fl32(min(max(x[m] - step (x_hi[m] - x_lo[m]) sgn(g[m]), x_lo[m]), x_hi[m]))   (sgn(0) = 0; fp64, then nearest fp32, moved inside the
//                                                                                        box if rounding left it)
// f(x') < best, strictly, makes it the best; not f(x') < f(x) stops the point (:110).  A point with a NaN among its coordinates, or whose
// f(x0) is NaN, takes no step.  A point that has stopped is masked: it is frozen, its accumulators still run (nobody reads them); a
// workgroup ends when all its points have stopped, or after n_steps.  Layer 0's activations ARE the current point (fp32 values held as
// doubles).  What the two entry points differ in is a compile-time choice of the wrapper (NetWalk), never a branch inside the loops:
//
//   NET_POINTS (gnnb_net_descend)          writes grad0 when asked, and computes that first gradient even where no step follows; a
//                                          point with a NaN coordinate reports the finite value its forward pass produced.
//   NET_STARTS (gnnb_net_descend_starts)   such a start's value IS a NaN (fmax in a ReLU would swallow it, and what is left is the
//                                          network's value at no point of the box): it never wins the pick.
//
// No atomics, no workgroup waits on another; every sum runs in a fixed order, so a point's result does not depend on B or on its row.

#define NET_THREADS KW_THREADS

struct NetArgs {
  KwNet net;
  const float* x; int n_starts;                         // (B, n_starts, N_0): the points; n_starts = 1 but for k_net_descend_tile
  const double* x_lo; const double* x_hi; const float* prop_w; const float* prop_b;     // (B, N_0) x 2, (B, N_L), (B)
  int n_steps; double step;
  float* xb; double* val; double* grad0; int32_t* steps_taken;  // per point: (., N_0), (.), null or (., N_0), null or (.)
  double* ws; long ws_stride;                           // per workgroup.  k_net_eval: 2 * `width`.  The descent: S x (the activations of graph layers 0..L, then two gradient buffers of `width`)
  int act_off[MAXL + 2], width;                         // act_off[k]: layer k's first activation; act_off[L + 1]: their total; width: the widest graph layer
};
static_assert(sizeof(NetArgs) <= 4096, "kernel arguments: 4 KiB");

static inline int net_eval_width(const KwNet& n) {
  int w = 1;
  for (int k = 0; k <= n.L; ++k) w = n.N[k] > w ? n.N[k] : w;
  return w;
}

static inline long net_descend_doubles(const KwNet& n) {
  long s = 0;
  for (int k = 0; k <= n.L; ++k) s += n.N[k];
  return s + 2L * net_eval_width(n);
}

// (A_k q)_j of a conv edge for S columns of q: the taps in dual_conv_at's order
template <int S>
__device__ __forceinline__ void net_conv_at(const KwEdge& E, int j, const double* q, double (&acc)[S]) {
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

// A_k^T nu at node m of the edge's input side for S columns of nu: kw_transpose_at over the whole output (y1, x1: its last row and
// column, E.h_out - 1 and E.w_out - 1, read once per layer by the caller), the taps in its order
template <int S>
__device__ __forceinline__ void net_transpose_at(const KwEdge& E, int m, const double* nu, int y1, int x1, double (&acc)[S]) {
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
  const int ntap = E.c_in * E.kh * E.kw, c_out = E.c_out;
  const long hwo = (long)E.h_out * E.w_out * S;
  for (int ky = 0; ky < E.kh; ++ky) {
    const int ty = iy + E.pad - ky;
    if (ty < 0 || ty % E.stride) continue;
    const int oy = ty / E.stride;
    if (oy > y1) continue;
    for (int kx = 0; kx < E.kw; ++kx) {
      const int tx = ix + E.pad - kx;
      if (tx < 0 || tx % E.stride) continue;
      const int ox = tx / E.stride;
      if (ox > x1) continue;
      const double* wp = w + ((long)ci * E.kh + ky) * E.kw + kx;
      const double* np = nu + ((long)oy * E.w_out + ox) * S;
      for (int co = 0; co < c_out; ++co) {
        const double c = wp[(long)co * ntap];
        const double* nq = np + co * hwo;
#pragma unroll
        for (int s = 0; s < S; ++s) acc[s] += c * nq[s];
      }
    }
  }
}

// Layers 1..L and the property row at S points by one workgroup: at(k) is where graph layer k's activations live, [node][S] (layer 0
// filled and synchronised by the caller).  f[s] = prop_w . act_L + prop_b on every thread.  red: S * NET_THREADS doubles of LDS.
template <int S, class At>
__device__ __forceinline__ void net_forward(const KwNet& net, const float* prop_w, float prop_b, At at, double* red, int tid, double (&f)[S]) {
  const int lane = tid & 63, wave = tid >> 6;
  for (int k = 1; k <= net.L; ++k) {
    const KwEdge& E = net.e[k];
    const int Nk = net.N[k];
    const double* cur = at(k - 1);
    double* nxt = at(k);
    if (E.kind == 0) {
      const int hw = E.h_out * E.w_out;
      for (int j = tid; j < Nk; j += NET_THREADS) {
        double acc[S];
        net_conv_at<S>(E, j, cur, acc);
        const double bias = E.bias[j / hw];
#pragma unroll
        for (int s = 0; s < S; ++s) nxt[(long)j * S + s] = fmax(acc[s] + bias, 0.0);
      }
    } else {
      for (int j = wave; j < Nk; j += NET_THREADS / 64) {
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
  for (int j = tid; j < NL; j += NET_THREADS) {
    const double c = (double)prop_w[j];
#pragma unroll
    for (int s = 0; s < S; ++s) f[s] += c * cur[(long)j * S + s];
  }
  kw_block_sum<S>(red, f, tid);
#pragma unroll
  for (int s = 0; s < S; ++s) f[s] = f[s] + (double)prop_b;
}

// g at S points from the activations `act` of their forward pass: returns the buffer (ga or gb) that holds the N_0 x S entries, synchronised
template <int S>
__device__ __forceinline__ double* net_backward(const NetArgs& a, const double* act, const float* prop_w, double* ga, double* gb, int tid) {
  const KwNet& net = a.net;
  const double* top = act + (long)a.act_off[net.L] * S;
  for (int j = tid; j < net.N[net.L]; j += NET_THREADS) {
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
    const int y1 = E.h_out - 1, x1 = E.w_out - 1;
    for (int m = tid; m < net.N[k - 1]; m += NET_THREADS) {     // (a gated node is exactly 0; the input layer has no gate)
      bool open[S], any = false;
#pragma unroll
      for (int s = 0; s < S; ++s) { open[s] = k == 1 || below[(long)m * S + s] > 0.0; any |= open[s]; }
      double acc[S];
      if (any) net_transpose_at<S>(E, m, cur, y1, x1, acc);
#pragma unroll
      for (int s = 0; s < S; ++s) nxt[(long)m * S + s] = open[s] ? acc[s] : 0.0;
    }
    double* t = cur; cur = nxt; nxt = t;
    __syncthreads();
  }
  return cur;
}

enum NetWalk { NET_POINTS, NET_STARTS };

// The descent of workgroup blockIdx.x: points s0 .. s0 + ns - 1 of row b (NET_POINTS: the one point of row b).  red: S * NET_THREADS doubles.
template <int S, NetWalk W>
__device__ __forceinline__ void net_descend(const NetArgs& a, double* red) {
  const int n = W == NET_STARTS ? a.n_starts : 1, tiles = (n + S - 1) / S;
  const int b = blockIdx.x / tiles, s0 = (blockIdx.x % tiles) * S, tid = threadIdx.x;
  const int ns = min(S, n - s0);                        // the last tile of a row may be partly empty: its empty columns carry a copy of column 0, masked
  const long p0 = (long)b * n + s0;
  const KwNet& net = a.net;
  const int N0 = net.N[0];
  double* act = a.ws + (long)blockIdx.x * a.ws_stride;
  double* ga = act + (long)a.act_off[net.L + 1] * S;
  double* gb = ga + (long)a.width * S;
  const float* x0 = a.x + p0 * N0;
  float* xb = a.xb + p0 * N0;
  const double* lo = a.x_lo + (long)b * N0;
  const double* hi = a.x_hi + (long)b * N0;
  const float* pw = a.prop_w + (long)b * net.N[net.L];
  const float pb = a.prop_b[b];
  const auto at = [&](int k) { return act + (long)a.act_off[k] * S; };
  int nanm = 0;
  for (int m = tid; m < N0; m += NET_THREADS) {
#pragma unroll
    for (int s = 0; s < S; ++s) {
      const float v = x0[(long)(s < ns ? s : 0) * N0 + m];
      if (s < ns) xb[(long)s * N0 + m] = v;             // best = (f(x0), x0), unconditionally
      act[(long)m * S + s] = (double)v;
      nanm |= (v != v) << s;
    }
  }
  bool on[S], nan[S];                                   // the points still descending; those with a NaN coordinate (the same on all threads)
#pragma unroll
  for (int s = 0; s < S; ++s) nan[s] = __syncthreads_or(nanm >> s & 1);
  double f[S], best[S], fn[S];
  int steps[S];
  net_forward<S>(net, pw, pb, at, red, tid, f);
  bool any = false;
#pragma unroll
  for (int s = 0; s < S; ++s) {
    best[s] = f[s];
    steps[s] = 0;
    on[s] = !nan[s] && s < ns && a.n_steps > 0 && f[s] == f[s];
    any |= on[s];
  }
  const double* g = nullptr;
  if (any || (W == NET_POINTS && a.grad0)) {
    g = net_backward<S>(a, act, pw, ga, gb, tid);
    if (W == NET_POINTS && a.grad0)
      for (int m = tid; m < N0; m += NET_THREADS)
#pragma unroll
        for (int s = 0; s < S; ++s)
          if (s < ns) a.grad0[(p0 + s) * N0 + m] = g[(long)m * S + s];
  }
  for (int t = 0; any && t < a.n_steps; ++t) {          // (f, best and so every branch below are the same on all threads)
    for (int m = tid; m < N0; m += NET_THREADS) {
      const double l = lo[m], h = hi[m];
#pragma unroll
      for (int s = 0; s < S; ++s) {
        if (!on[s]) continue;                           // a stopped point is frozen
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
    net_forward<S>(net, pw, pb, at, red, tid, fn);
    any = false;
#pragma unroll
    for (int s = 0; s < S; ++s) {
      if (!on[s]) continue;
      ++steps[s];
      if (fn[s] < best[s]) {
        best[s] = fn[s];
        for (int m = tid; m < N0; m += NET_THREADS) xb[(long)s * N0 + m] = (float)act[(long)m * S + s];
      }
      if (!(fn[s] < f[s])) on[s] = false;               // the reference's stop rule; a NaN stops here too
      else f[s] = fn[s];
      any |= on[s];
    }
    if (any && t + 1 < a.n_steps) g = net_backward<S>(a, act, pw, ga, gb, tid);
  }
  if (tid == 0) {
#pragma unroll
    for (int s = 0; s < S; ++s) {
      if (s >= ns) continue;
      a.val[p0 + s] = W == NET_STARTS && nan[s] ? __builtin_nan("") : best[s];      // (a ReLU's fmax swallows a NaN: the value left is no upper bound)
      if (a.steps_taken) a.steps_taken[p0 + s] = steps[s];
    }
  }
}

__global__ __launch_bounds__(NET_THREADS) void k_net_eval(NetArgs a) {
  __shared__ double red[NET_THREADS];
  const int b = blockIdx.x, tid = threadIdx.x;
  double* buf = a.ws + (long)b * a.ws_stride;
  const int N0 = a.net.N[0];
  for (int m = tid; m < N0; m += NET_THREADS) buf[m] = (double)a.x[(long)b * N0 + m];
  __syncthreads();
  double f[1];
  net_forward<1>(a.net, a.prop_w + (long)b * a.net.N[a.net.L], a.prop_b[b], [&](int k) { return buf + (k & 1) * (long)a.width; }, red, tid, f);
  if (tid == 0) a.val[b] = f[0];
}

__global__ __launch_bounds__(NET_THREADS) void k_net_descend(NetArgs a) {
  __shared__ double red[NET_THREADS];
  net_descend<1, NET_POINTS>(a, red);
}

template <int S>
__global__ __launch_bounds__(NET_THREADS) void k_net_descend_tile(NetArgs a) {
  __shared__ double red[S * NET_THREADS];
  net_descend<S, NET_STARTS>(a, red);
}
