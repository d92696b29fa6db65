// gnnb_k_kw.h -- Wong-Kolter intermediate bounds of a batch of BaB domains, fp64 (gnnb_kw_bounds).
//
// Restates gnn_branching_amd/lp_producer.py LayerGraphLP.kw_bounds / _kw_layer, which restate the reference's
// init_kw_bounds / update_kw_bounds (plnn/dual_network_linear_approximation.py:205-294, :296-451) on the dual network of
// convex_adversarial/dual_network.py:15-121.  The bound network is x -> A_1 -> ReLU -> ... -> A_L -> ReLU -> A_{L+1} with
// A_{L+1} the per-domain property layer; graph layer k (1..L+1) is the output of A_k.  Layers go in order, one launch per
// layer (layer k reads the finished bounds of every layer below it):
//
//   * k_kw_first   graph layer 1: interval image of the input box (exact for one affine map), one thread per node; also the
//                  fp32 copy of the box and the fp64 copy of the property layer's weights.
//   * k_kw_layer   graph layer k >= 2: one workgroup per (node j, domain b).  The interval image of node j under A_k, and the
//                  KW backward pass of direction e_j: nu <- A_k^T e_j, then per ReLU layer i = k-1 .. 1 the gains
//                  (-d l) min(nu, 0) / (-d l) max(nu, 0) over the ambiguous set, nu <- d nu, the bias gain nu . b_i and
//                  nu <- A_i^T nu; at the input the box terms.  nu lives in LDS (two buffers of the widest ReLU layer).  Below a
//                  conv node nu is zero outside the node's receptive field: every step works on the spatial box of rows and
//                  columns that hold its support (all channels; the whole layer once a Linear map is crossed) and treats the
//                  rest as the zeros it is (base, conv-2 node: 16 x 4 x 4 of 2048 layer-1 nodes, 3 x 10 x 10 of 3072 inputs).
//   * k_kw_flag    per domain: lo > up + 1e-9 anywhere (the test LayerGraphLP.solve applies before its LP).
//
// Every layer's bounds are then intersected with the parent's (when the domain has one), the split mask is applied to the
// pre-activation bounds, and the ReLU relaxation (d, -d l) of each node is stored for the passes above it.  Up to the split
// layer a child takes its parent's bounds unchanged (update_kw_bounds' incremental form).  Each workgroup reduces in a
// fixed order (per-thread partials, then a fixed tree): a domain's bounds do not depend on B or on its place in the batch.
// No float atomics, no workgroup waits on another, no allocation.

#define KW_THREADS 256

static inline size_t kw_lds_doubles(int maxNr) { return (size_t)(2 * maxNr > 5 * KW_THREADS ? 2 * maxNr : 5 * KW_THREADS); }

struct KwEdge : EdgeGeom {      // (gnnb_pack.h: kind, the conv geometry, n_in, n_out)
  const double* w;              // conv: [co][ci][ky][kx]; linear: [o][i] (torch layout), fp64
  const double* bias;           // per output channel (conv) / node (linear)
  long wb, bb;                  // per-domain strides of w / bias in doubles (0: shared; the property layer: N_L + 1)
};

struct KwNet {                  // the bound network as the fp64 kernels read it: made once by gnnb_bind_network, copied into every call's arguments
  KwEdge e[MAXL + 2];                                   // e[k]: the map into graph layer k, k = 1..L (e[L + 1], the property layer: gnnb_kw_bounds, per call)
  int N[MAXL + 2], off[MAXL + 2];                       // nodes of graph layer k; off[k]: flat ReLU index of layer k's first node
  int lc[MAXL + 2], lh[MAXL + 2], lw[MAXL + 2];         // graph layer k as (C, H, W) (a Linear map's output: (N_k, 1, 1)), k = 0..L
  int L, R, maxNr;                                      // maxNr: widest ReLU layer (LDS buffers)
};

struct KwArgs {
  KwNet net; int B;                                     // (net.e[L + 1]: this call's property layer); domains
  double* lb[MAXL + 2]; double* ub[MAXL + 2];           // outputs, graph layers 1..L+1, (B, N_k)
  float* lb32[MAXL + 2]; float* ub32[MAXL + 2];         // optional fp32 copies, graph layers 0..L+1 (layer 0 = box)
  const double* plb[MAXL + 2]; const double* pub[MAXL + 2];   // parent bounds, graph layers 1..L+1 (null: no parents)
  const double* x_lo; const double* x_hi;               // (B, N_0)
  const float* prop_w; const float* prop_b;             // (B, N_L), (B)
  const int8_t* mask;                                   // (B, R), {-1, 0, 1}
  const int32_t* split;                                 // (B): ReLU layer of the split that made the domain, -1 = no parent; may be null
  double* dg;                                           // workspace (B, R, 2): d and -d l of every ReLU node, mask applied
  double* pw;                                           // workspace (B, N_L + 1): property weights then bias, fp64
  int32_t* infeasible;                                  // (B)
};

// upper relaxation s p + t of an ambiguous ReLU with pre-activation bounds l < 0 < u
__device__ __forceinline__ void kw_relax(double l, double u, double& s, double& t) {
  s = u / fmax(u - l, 1e-300);
  t = -l * s;
}

// sums of v[0..NV) over the workgroup, left in v on every thread: per-thread partials in, then a fixed tree.  red: NV * KW_THREADS
// doubles of LDS that nobody else is using (synchronises before and after)
template <int NV>
__device__ __forceinline__ void kw_block_sum(double* red, double* v, int tid) {
  __syncthreads();
  for (int r = 0; r < NV; ++r) red[r * KW_THREADS + tid] = v[r];
  __syncthreads();
  for (int s = KW_THREADS / 2; s > 0; s >>= 1) {
    if (tid < s)
      for (int r = 0; r < NV; ++r) red[r * KW_THREADS + tid] += red[r * KW_THREADS + tid + s];
    __syncthreads();
  }
  for (int r = 0; r < NV; ++r) v[r] = red[r * KW_THREADS];
  __syncthreads();
}

struct KwBox {                  // all channels x rows y0..y1 x columns x0..x1 of a graph layer laid out (C, H, W): where nu can be non-zero
  int y0, y1, x0, x1;
  __device__ __forceinline__ int count(int C) const { return C * (y1 - y0 + 1) * (x1 - x0 + 1); }
  // node of the box's t-th entry (channel-major, then rows, then columns)
  __device__ __forceinline__ int node(int t, int H, int W) const {
    const int bh = y1 - y0 + 1, bw = x1 - x0 + 1, c = t / (bh * bw), r = t % (bh * bw);
    return (c * H + y0 + r / bw) * W + x0 + r % bw;
  }
  // the box of E's input layer (H x W) that holds the support of A^T nu: the receptive fields of a conv, the whole layer of a Linear map
  __device__ __forceinline__ KwBox below(const KwEdge& E, int H, int W) const {
    if (E.kind != 0) return KwBox{0, H - 1, 0, W - 1};
    return KwBox{max(0, y0 * E.stride - E.pad), min(H - 1, y1 * E.stride - E.pad + E.kh - 1),
                 max(0, x0 * E.stride - E.pad), min(W - 1, x1 * E.stride - E.pad + E.kw - 1)};
  }
};

__device__ __forceinline__ bool kw_has_parent(const KwArgs& a, int b) {
  return a.plb[1] != nullptr && a.split != nullptr && a.split[b] >= 0;
}

// a child keeps its parent's bounds of graph layers 1..split+1; a split_layer past the last ReLU layer counts as the last one, so
// the property layer (graph layer L+1) is always recomputed
__device__ __forceinline__ bool kw_copies(const KwArgs& a, int b, int k) {
  return kw_has_parent(a, b) && k <= min(a.split[b], a.net.L - 1) + 1;
}

// node j of graph layer k in domain b: parent intersection (or copy), split mask, outputs, ReLU relaxation
__device__ void kw_finish(const KwArgs& a, int k, int b, int j, double nl, double nu) {
  const int Nk = a.net.N[k];
  const long at = (long)b * Nk + j;
  if (kw_copies(a, b, k)) {
    nl = a.plb[k][at];
    nu = a.pub[k][at];
  } else if (kw_has_parent(a, b)) {
    nl = fmax(nl, a.plb[k][at]);
    nu = fmin(nu, a.pub[k][at]);
  }
  if (k <= a.net.L) {
    const int m = a.mask[(long)b * a.net.R + a.net.off[k] + j];
    if (m == 1) nl = fmax(nl, 0.0);
    if (m == 0) nu = fmin(nu, 0.0);
    double d = nl >= 0.0 ? 1.0 : 0.0, g = 0.0;              // (d, -d l) of the relaxation the passes above read
    if (nl < 0.0 && nu > 0.0) kw_relax(nl, nu, d, g);
    double* dg = a.dg + ((long)b * a.net.R + a.net.off[k] + j) * 2;
    dg[0] = d;
    dg[1] = g;
  }
  a.lb[k][at] = nl;
  a.ub[k][at] = nu;
  if (a.lb32[k]) {
    a.lb32[k][at] = (float)nl;
    a.ub32[k][at] = (float)nu;
  }
}

// interval image of node j of E over [lo, up] (post-ReLU bounds, or the box): partial sums of the taps t = t0, t0 + dt, ...
__device__ __forceinline__ void kw_interval_part(const KwEdge& E, int b, int j, const double* lo, const double* up, bool relu_in, int t0,
                                                 int dt, double& al, double& au) {
  const double* w = E.w + (long)b * E.wb;
  if (E.kind == 1) {
    const double* row = w + (long)j * E.n_in;
    for (int t = t0; t < E.n_in; t += dt) {
      const double c = row[t];
      double l = lo[t], u = up[t];
      if (relu_in) { l = fmax(l, 0.0); u = fmax(u, 0.0); }
      if (c >= 0.0) { al += c * l; au += c * u; } else { al += c * u; au += c * l; }
    }
    return;
  }
  const int hw = E.h_out * E.w_out, co = j / hw, oy = (j % hw) / E.w_out, ox = j % E.w_out;
  const int ntap = E.c_in * E.kh * E.kw;
  for (int t = t0; t < ntap; t += dt) {
    const int ci = t / (E.kh * E.kw), ky = (t / E.kw) % E.kh, kx = t % E.kw;
    const int iy = oy * E.stride - E.pad + ky, ix = ox * E.stride - E.pad + kx;
    if (iy < 0 || iy >= E.h_in || ix < 0 || ix >= E.w_in) continue;
    const double c = w[(long)co * ntap + t];
    const long s = ((long)ci * E.h_in + iy) * E.w_in + ix;
    double l = lo[s], u = up[s];
    if (relu_in) { l = fmax(l, 0.0); u = fmax(u, 0.0); }
    if (c >= 0.0) { al += c * l; au += c * u; } else { al += c * u; au += c * l; }
  }
}

__device__ __forceinline__ double kw_bias_of(const KwEdge& E, int b, int j) {
  return E.bias[(long)b * E.bb + (E.kind == 0 ? j / (E.h_out * E.w_out) : j)];
}

// graph layer 1, one thread per (node, domain); the same threads also write the fp32 box and the fp64 property weights
__global__ __launch_bounds__(KW_THREADS) void k_kw_first(KwArgs a, int span) {
  const long gid = (long)blockIdx.x * KW_THREADS + threadIdx.x;
  if (gid >= (long)span * a.B) return;
  const int b = (int)(gid / span), n = (int)(gid % span);
  const int N0 = a.net.N[0], NL = a.net.N[a.net.L];
  if (n < N0 && a.lb32[0]) {
    a.lb32[0][(long)b * N0 + n] = (float)a.x_lo[(long)b * N0 + n];
    a.ub32[0][(long)b * N0 + n] = (float)a.x_hi[(long)b * N0 + n];
  }
  if (n < NL) a.pw[(long)b * (NL + 1) + n] = (double)a.prop_w[(long)b * NL + n];
  if (n == NL) a.pw[(long)b * (NL + 1) + NL] = (double)a.prop_b[b];
  if (n < a.net.N[1]) {
    double al = 0.0, au = 0.0;
    if (!kw_copies(a, b, 1)) {
      const KwEdge& E = a.net.e[1];
      kw_interval_part(E, b, n, a.x_lo + (long)b * N0, a.x_hi + (long)b * N0, false, 0, 1, al, au);
      const double c = kw_bias_of(E, b, n);
      al += c;
      au += c;
    }
    kw_finish(a, 1, b, n, al, au);
  }
}

// A_i^T nu at node m of the map's input side (nu: A_i's output, in LDS, zero outside rows y0..y1 / columns x0..x1)
__device__ __forceinline__ double kw_transpose_at(const KwEdge& E, int b, int m, const double* nu, int y0, int y1, int x0, int x1) {
  const double* w = E.w + (long)b * E.wb;
  double acc = 0.0;
  if (E.kind == 1) {
    for (int o = 0; o < E.n_out; ++o) acc += w[(long)o * E.n_in + m] * nu[o];
    return acc;
  }
  const int hwi = E.h_in * E.w_in, ci = m / hwi, iy = (m % hwi) / E.w_in, ix = m % E.w_in;
  const int ntap = E.c_in * E.kh * E.kw;
  for (int ky = 0; ky < E.kh; ++ky) {
    const int ty = iy + E.pad - ky;
    if (ty < 0 || ty % E.stride) continue;
    const int oy = ty / E.stride;
    if (oy < y0 || oy > y1) continue;
    for (int kx = 0; kx < E.kw; ++kx) {
      const int tx = ix + E.pad - kx;
      if (tx < 0 || tx % E.stride) continue;
      const int ox = tx / E.stride;
      if (ox < x0 || ox > x1) continue;
      const double* wp = w + ((long)ci * E.kh + ky) * E.kw + kx;
      const double* np = nu + (long)oy * E.w_out + ox;
      for (int co = 0; co < E.c_out; ++co) acc += wp[(long)co * ntap] * np[(long)co * E.h_out * E.w_out];
    }
  }
  return acc;
}

// A_k^T e_j at node m of A_k's input side: the weight that joins m to node j, or 0
__device__ __forceinline__ double kw_row_at(const KwEdge& E, int b, int j, int m) {
  const double* w = E.w + (long)b * E.wb;
  if (E.kind == 1) return w[(long)j * E.n_in + m];
  const int hw = E.h_out * E.w_out, co = j / hw, oy = (j % hw) / E.w_out, ox = j % E.w_out;
  const int hwi = E.h_in * E.w_in, ci = m / hwi, iy = (m % hwi) / E.w_in, ix = m % E.w_in;
  const int ky = iy + E.pad - oy * E.stride, kx = ix + E.pad - ox * E.stride;
  if (ky < 0 || ky >= E.kh || kx < 0 || kx >= E.kw) return 0.0;
  return w[(((long)co * E.c_in + ci) * E.kh + ky) * E.kw + kx];
}

// graph layer k >= 2: one workgroup per (node j, domain b)
__global__ __launch_bounds__(KW_THREADS) void k_kw_layer(KwArgs a, int k) {
  const int j = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  if (kw_copies(a, b, k)) {
    if (tid == 0) kw_finish(a, k, b, j, 0.0, 0.0);
    return;
  }
  extern __shared__ double kw_lds[];
  const KwNet& net = a.net;
  double* cur = kw_lds;
  double* nxt = kw_lds + net.maxNr;
  const KwEdge& E = net.e[k];
  double il = 0.0, iu = 0.0, sl = 0.0, su = 0.0, sc = 0.0;
  // interval image of node j over the post-ReLU bounds of layer k-1
  kw_interval_part(E, b, j, a.lb[k - 1] + (long)b * net.N[k - 1], a.ub[k - 1] + (long)b * net.N[k - 1], true, tid, KW_THREADS, il, iu);
  // support box of nu in layer k-1: the receptive field of node j (a conv node) or the whole layer
  const int oy = E.kind == 0 ? (j % (E.h_out * E.w_out)) / E.w_out : 0, ox = E.kind == 0 ? j % E.w_out : 0;
  KwBox box = KwBox{oy, oy, ox, ox}.below(E, net.lh[k - 1], net.lw[k - 1]);
  // nu = A_k^T e_j (its bias gain b_k[j] is added after the reduction)
  for (int t = tid, nb = box.count(net.lc[k - 1]); t < nb; t += KW_THREADS) {
    const int m = box.node(t, net.lh[k - 1], net.lw[k - 1]);
    cur[m] = kw_row_at(E, b, j, m);
  }
  for (int i = k - 1; i >= 1; --i) {
    __syncthreads();
    // ReLU of layer i: gains over the ambiguous set, nu <- d nu; then the bias gain of A_i (box nodes only: nu is 0 elsewhere)
    const double* dg = a.dg + ((long)b * net.R + net.off[i]) * 2;
    const KwEdge& Ei = net.e[i];
    const int hw = Ei.kind == 0 ? Ei.h_out * Ei.w_out : 1;
    for (int t = tid, nb = box.count(net.lc[i]); t < nb; t += KW_THREADS) {
      const int m = box.node(t, net.lh[i], net.lw[i]);
      const double v = cur[m], d = dg[2 * m], g = dg[2 * m + 1];
      sl += fmin(v, 0.0) * g;
      su += fmax(v, 0.0) * g;
      const double nv = v * d;
      cur[m] = nv;
      sc += nv * Ei.bias[(long)b * Ei.bb + m / hw];
    }
    __syncthreads();
    const KwBox in = box.below(Ei, net.lh[i - 1], net.lw[i - 1]);      // support box in layer i-1
    const int nb = in.count(net.lc[i - 1]);
    if (i > 1) {
      for (int t = tid; t < nb; t += KW_THREADS) {
        const int m = in.node(t, net.lh[i - 1], net.lw[i - 1]);
        nxt[m] = kw_transpose_at(Ei, b, m, cur, box.y0, box.y1, box.x0, box.x1);
      }
      double* t = cur; cur = nxt; nxt = t;
    } else {                                  // the input: box terms
      const double* xl = a.x_lo + (long)b * net.N[0];
      const double* xu = a.x_hi + (long)b * net.N[0];
      for (int t = tid; t < nb; t += KW_THREADS) {
        const int m = in.node(t, net.lh[0], net.lw[0]);
        const double v = kw_transpose_at(Ei, b, m, cur, box.y0, box.y1, box.x0, box.x1), vp = fmax(v, 0.0), vn = fmin(v, 0.0);
        sl += vp * xl[m] + vn * xu[m];
        su += vp * xu[m] + vn * xl[m];
      }
    }
    box = in;
  }
  double sum[5] = {il, iu, sl, su, sc};       // the nu buffers become the reduction's (kw_lds_doubles: >= 5 KW_THREADS)
  kw_block_sum<5>(kw_lds, sum, tid);
  if (tid == 0) {
    const double c = kw_bias_of(E, b, j);
    const double kl = c + sum[4] + sum[2], ku = c + sum[4] + sum[3];
    const double nl = fmax(sum[0] + c, kl), nu = fmin(sum[1] + c, ku);
    kw_finish(a, k, b, j, nl, nu);
  }
}

// per domain: 1 where some bound pair is crossed by more than 1e-9 (box and graph layers; the post-ReLU and flattened
// entries of the host's list cross only where their pre-activation does)
__global__ __launch_bounds__(KW_THREADS) void k_kw_flag(KwArgs a) {
  const int b = blockIdx.x, tid = threadIdx.x;
  int bad = 0;
  for (int n = tid; n < a.net.N[0]; n += KW_THREADS) bad |= a.x_lo[(long)b * a.net.N[0] + n] > a.x_hi[(long)b * a.net.N[0] + n] + 1e-9;
  for (int k = 1; k <= a.net.L + 1; ++k)
    for (int n = tid; n < a.net.N[k]; n += KW_THREADS) bad |= a.lb[k][(long)b * a.net.N[k] + n] > a.ub[k][(long)b * a.net.N[k] + n] + 1e-9;
  bad = __syncthreads_or(bad);
  if (tid == 0) a.infeasible[b] = bad ? 1 : 0;
}
