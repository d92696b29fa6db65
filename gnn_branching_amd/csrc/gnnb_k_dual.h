// gnnb_k_dual.h -- lower bounds of a batch of BaB domains by dual ascent, fp64 (gnnb_dual_ascent).
//
// Restates gnn_branching_amd/lp_producer.py LayerGraphLP.dual_value / dual_ascent_host / dual_recover.  With the
// intermediate bounds (l, u) of gnnb_kw_bounds fixed, the dual of the subproblem LP (reference plnn/conv_kwinter_gen.py:179-555) is the
// Wong-Kolter dual network of gnnb_k_kw.h with two changes: the slope alpha in [0, 1] of every ambiguous ReLU's lower relaxation is free
// (k_kw_layer fixes it to u / (u - l)), and every split node carries one multiplier beta >= 0 of its clamp.  Every (alpha, beta) gives a
// sound lower bound g(alpha, beta) on the property output; the maximum over them is the LP optimum.
//
//   * k_dual_ascent   one workgroup per domain, every iteration in one launch:
//       backward   lambda_L = property weights, c = property bias; per ReLU layer k = L..1 the node rule
//                  (ambiguous: mu = lambda alpha if lambda >= 0, else mu = lambda s and c += lambda t; passing: mu = lambda; blocked:
//                  mu = 0; mask 1: mu -= beta, mask 0: mu += beta; c += mu b_k) and lambda_{k-1} = A_k^T mu (kw_transpose_at over
//                  the whole layer); at the input c += lambda_0 x_lo (lambda_0 >= 0) or lambda_0 x_hi.  g = c.  lambda lives in
//                  LDS (two buffers of the widest ReLU layer); each layer's lambda and the minimiser x* go to the workspace.
//       forward    the exact supergradient: p_k = A_k q_{k-1} + b_k from q_0 = x*, q_k the linearised ReLU the backward pass chose;
//                  d g / d alpha = max(lambda, 0) p on ambiguous nodes, d g / d beta = -p (mask 1) / +p (mask 0).  The thread that
//                  computes a node's p also takes its Adam step (ascent; b1 0.9, b2 0.999, eps 1e-8, moments in the workspace) and
//                  projects alpha onto [0, 1], beta onto [0, inf).
//       recovery   once more at the best (alpha, beta): the forward pass propagating the ENVELOPE value of every ReLU (max(p, 0) where
//                  lambda >= 0, s p + t where lambda < 0), which is a point of the relaxation, written as gnnb_batch's fp32 arrays.
//
// Reductions are per-thread partials in a fixed node order, then a fixed tree (a Linear row: 64 lanes, then a fixed butterfly): a
// domain's result does not depend on B or on its place in the batch.  No float atomics, no workgroup waits on another, no allocation.

#define DUAL_THREADS KW_THREADS

struct DualArgs {
  KwNet net;                                            // e[k], k = 1..L, and graph layers 0..L (the property layer is read as prop_w / prop_b)
  int n_iter, warm;
  double lr;
  const double* lb[MAXL + 2]; const double* ub[MAXL + 2];   // pre-activation bounds of graph layers 1..L, (B, N_k), mask applied
  const double* x_lo; const double* x_hi;               // (B, N_0)
  const float* prop_w; const float* prop_b;             // (B, N_L), (B)
  const int8_t* mask;                                   // (B, R)
  double* alpha; double* beta;                          // (B, R) in/out
  double* bound;                                        // (B)
  double* grad_alpha; double* grad_beta;                // null, or (B, R): the supergradient at the entry point
  float* dual[MAXL + 2]; float* z_pre[MAXL + 2]; float* z_post[MAXL + 2];   // null, or the scorer's inputs of ReLU layer k = 1..L
  float* z_out; float* x_lp; float* lb32_prop;          // (B), (B, N_0), (B)
  double* ws; long ws_stride;                           // workspace, ws_stride doubles per domain (dual_ws_doubles)
};
static_assert(sizeof(KwArgs) <= 4096 && sizeof(DualArgs) <= 4096, "kernel arguments are passed by value: HIP's limit is 4 KiB");

// per domain, in doubles: lambda (R), x* (N_0), Adam's first and second moments of alpha and beta (4 R), the best (alpha, beta) (2 R)
static inline size_t dual_ws_doubles(int R, int N0) { return (size_t)7 * R + N0; }

// state of a ReLU node: 0 ambiguous (s, t: the upper relaxation s p + t), 1 passing, 2 blocked
__device__ __forceinline__ int dual_state(int m, double l, double u, double& s, double& t) {
  s = 0.0; t = 0.0;
  if (m == 1) return 1;
  if (m == 0) return 2;
  if (l >= 0.0) return 1;
  if (!(u > 0.0)) return 2;
  kw_relax(l, u, s, t);
  return 0;
}

// g(alpha, beta) of domain b; leaves lambda_k of every ReLU node and the minimiser x* in the workspace
__device__ double dual_backward(const DualArgs& a, int b, int tid, double* lds, double* lam_ws, double* xs) {
  double* cur = lds;
  double* nxt = lds + a.net.maxNr;
  const double* al = a.alpha + (long)b * a.net.R;
  const double* be = a.beta + (long)b * a.net.R;
  const int8_t* mask = a.mask + (long)b * a.net.R;
  double c = tid == 0 ? (double)a.prop_b[b] : 0.0;
  for (int k = a.net.L; k >= 1; --k) {
    const KwEdge& E = a.net.e[k];
    const int Nk = a.net.N[k], hw = E.kind == 0 ? E.h_out * E.w_out : 1;
    const double* lo = a.lb[k] + (long)b * Nk;
    const double* up = a.ub[k] + (long)b * Nk;
    for (int j = tid; j < Nk; j += DUAL_THREADS) {
      const int r = a.net.off[k] + j, m = mask[r];
      const double lam = k == a.net.L ? (double)a.prop_w[(long)b * Nk + j] : cur[j];
      double s, t, mu;
      const int st = dual_state(m, lo[j], up[j], s, t);
      if (st == 0) {
        if (lam >= 0.0) mu = lam * al[r];
        else { mu = lam * s; c += lam * t; }
      } else {
        mu = st == 1 ? lam : 0.0;
      }
      if (m == 1) mu -= be[r];
      if (m == 0) mu += be[r];
      c += mu * E.bias[j / hw];
      lam_ws[r] = lam;
      cur[j] = mu;
    }
    __syncthreads();
    const int Nin = a.net.N[k - 1], y1 = a.net.lh[k] - 1, x1 = a.net.lw[k] - 1;
    if (k > 1) {
      for (int m = tid; m < Nin; m += DUAL_THREADS) nxt[m] = kw_transpose_at(E, 0, m, cur, 0, y1, 0, x1);
      double* t = cur; cur = nxt; nxt = t;
      __syncthreads();
    } else {
      const double* xl = a.x_lo + (long)b * Nin;
      const double* xu = a.x_hi + (long)b * Nin;
      for (int m = tid; m < Nin; m += DUAL_THREADS) {
        const double v = kw_transpose_at(E, 0, m, cur, 0, y1, 0, x1);
        const double x = v >= 0.0 ? xl[m] : xu[m];
        c += v * x;
        xs[m] = x;
      }
    }
  }
  kw_block_sum<1>(lds, &c, tid);
  return c;
}

// (A_k q)_j of a conv edge of domain b, one thread per node; q holds rows y0.. / columns x0.. of every input channel, qh x qw per channel
__device__ __forceinline__ double dual_conv_window_at(const KwEdge& E, int b, int j, const double* q, int y0, int x0, int qh, int qw) {
  const int hw = E.h_out * E.w_out, co = j / hw, oy = (j % hw) / E.w_out, ox = j % E.w_out;
  const double* w = E.w + (long)b * E.wb + (long)co * E.c_in * E.kh * E.kw;
  double acc = 0.0;
  for (int ci = 0; ci < E.c_in; ++ci)
    for (int ky = 0; ky < E.kh; ++ky) {
      const int iy = oy * E.stride - E.pad + ky;
      if (iy < 0 || iy >= E.h_in) continue;
      for (int kx = 0; kx < E.kw; ++kx) {
        const int ix = ox * E.stride - E.pad + kx;
        if (ix < 0 || ix >= E.w_in) continue;
        acc += w[(ci * E.kh + ky) * E.kw + kx] * q[((long)ci * qh + iy - y0) * qw + ix - x0];
      }
    }
  return acc;
}

// ... of a shared edge over the whole input layer
__device__ __forceinline__ double dual_conv_at(const KwEdge& E, int j, const double* q) {
  return dual_conv_window_at(E, 0, j, q, 0, 0, E.h_in, E.w_in);
}

enum { DUAL_STEP = 1, DUAL_GRAD = 2, DUAL_RECOVER = 4 };

// node j of ReLU layer k with pre-activation p: what the forward pass leaves behind; returns q_k[j]
__device__ __forceinline__ double dual_node(const DualArgs& a, int b, int k, int j, double p, int what, double bc1, double bc2) {
  const int r = a.net.off[k] + j;
  const long at = (long)b * a.net.R + r;
  double* ws = a.ws + (long)b * a.ws_stride;
  const int m = a.mask[at];
  const double lam = ws[r];
  double s, t;
  const int st = dual_state(m, a.lb[k][(long)b * a.net.N[k] + j], a.ub[k][(long)b * a.net.N[k] + j], s, t);
  const double al = a.alpha[at];
  double q = st == 1 ? p : 0.0;
  if (st == 0) q = lam >= 0.0 ? al * p : s * p + t;
  const double ga = st == 0 ? fmax(lam, 0.0) * p : 0.0;
  const double gb = m == 1 ? -p : (m == 0 ? p : 0.0);
  if (what & DUAL_GRAD) {
    a.grad_alpha[at] = ga;
    a.grad_beta[at] = gb;
  }
  if (what & DUAL_STEP) {
    const double b1 = 0.9, b2 = 0.999, omb1 = 1.0 - b1, omb2 = 1.0 - b2, eps = 1e-8;
    double* mom = ws + a.net.R + a.net.N[0];                    // m_alpha, v_alpha, m_beta, v_beta: R doubles each
    const double ma = b1 * mom[r] + omb1 * ga, va = b2 * mom[a.net.R + r] + omb2 * (ga * ga);
    const double mb = b1 * mom[2 * a.net.R + r] + omb1 * gb, vb = b2 * mom[3 * a.net.R + r] + omb2 * (gb * gb);
    mom[r] = ma; mom[a.net.R + r] = va; mom[2 * a.net.R + r] = mb; mom[3 * a.net.R + r] = vb;
    a.alpha[at] = fmin(fmax(al + a.lr * ((ma / bc1) / (sqrt(va / bc2) + eps)), 0.0), 1.0);
    a.beta[at] = fmax(a.beta[at] + a.lr * ((mb / bc1) / (sqrt(vb / bc2) + eps)), 0.0);
  }
  if (what & DUAL_RECOVER) {
    if (st == 0 && lam >= 0.0) q = fmax(p, 0.0);        // the envelope value, not the linearised one
    if (a.dual[k]) {
      const long n = (long)b * a.net.N[k] + j;
      a.z_pre[k][n] = (float)p;
      a.z_post[k][n] = (float)q;
      a.dual[k][3 * n] = 0.0f;
      a.dual[k][3 * n + 1] = st == 0 ? (float)(al * fmax(lam, 0.0)) : 0.0f;
      a.dual[k][3 * n + 2] = st == 0 ? (float)fmin(lam, 0.0) : 0.0f;
    }
  }
  return q;
}

// the forward pass at the point the last dual_backward evaluated (its lambda and x* are in the workspace)
__device__ void dual_forward(const DualArgs& a, int b, int tid, double* lds, const double* xs, int what, double bc1, double bc2) {
  double* cur = lds;
  double* nxt = lds + a.net.maxNr;
  const int lane = tid & 63, wave = tid >> 6;
  for (int k = 1; k <= a.net.L; ++k) {
    const KwEdge& E = a.net.e[k];
    const int Nk = a.net.N[k];
    const double* q = k == 1 ? xs : cur;
    double* out = k == 1 ? cur : nxt;
    if (E.kind == 0) {
      const int hw = E.h_out * E.w_out;
      for (int j = tid; j < Nk; j += DUAL_THREADS) out[j] = dual_node(a, b, k, j, dual_conv_at(E, j, q) + E.bias[j / hw], what, bc1, bc2);
    } else {                                            // a Linear row per wave: lanes walk the row coalesced, then a fixed butterfly
      for (int j = wave; j < Nk; j += DUAL_THREADS / 64) {
        const double* row = E.w + (long)j * E.n_in;
        double acc = 0.0;
        for (int t = lane; t < E.n_in; t += 64) acc += row[t] * q[t];
        for (int s = 32; s > 0; s >>= 1) acc += __shfl_xor(acc, s, 64);
        if (lane == 0) out[j] = dual_node(a, b, k, j, acc + E.bias[j], what, bc1, bc2);
      }
    }
    if (k > 1) { double* t = cur; cur = nxt; nxt = t; }
    __syncthreads();
  }
  if (what & DUAL_RECOVER) {
    const int NL = a.net.N[a.net.L], N0 = a.net.N[0];
    double part = 0.0;
    for (int j = tid; j < NL; j += DUAL_THREADS) part += (double)a.prop_w[(long)b * NL + j] * cur[j];
    kw_block_sum<1>(lds, &part, tid);                   // (every thread has read its q before the buffer becomes the tree's)
    if (a.dual[1]) {
      if (tid == 0) a.z_out[b] = (float)(part + (double)a.prop_b[b]);
      for (int m = tid; m < N0; m += DUAL_THREADS) a.x_lp[(long)b * N0 + m] = (float)xs[m];
    }
  }
}

__global__ __launch_bounds__(DUAL_THREADS) void k_dual_ascent(DualArgs a) {
  extern __shared__ double dual_lds[];
  const int b = blockIdx.x, tid = threadIdx.x, R = a.net.R;
  double* ws = a.ws + (long)b * a.ws_stride;
  double* lam_ws = ws;
  double* xs = ws + R;
  double* mom = xs + a.net.N[0];
  double* best_pt = mom + 4 * (long)R;
  double* al = a.alpha + (long)b * R;
  double* be = a.beta + (long)b * R;
  // entry point: the projection of the caller's (warm) or alpha = u / (u - l), beta = 0; Adam's moments start at zero
  for (int k = 1; k <= a.net.L; ++k)
    for (int j = tid; j < a.net.N[k]; j += DUAL_THREADS) {
      const int r = a.net.off[k] + j, m = a.mask[(long)b * R + r];
      double s, t;
      const int st = dual_state(m, a.lb[k][(long)b * a.net.N[k] + j], a.ub[k][(long)b * a.net.N[k] + j], s, t);
      al[r] = a.warm ? fmin(fmax(al[r], 0.0), 1.0) : (st == 0 ? s : 0.0);
      be[r] = a.warm && m != -1 ? fmax(be[r], 0.0) : 0.0;
      mom[r] = 0.0; mom[R + r] = 0.0; mom[2 * R + r] = 0.0; mom[3 * R + r] = 0.0;
    }
  __syncthreads();
  double best = 0.0, b1t = 1.0, b2t = 1.0;
  for (int it = 0;; ++it) {
    const double g = dual_backward(a, b, tid, dual_lds, lam_ws, xs);
    if (it == 0 || g > best) {
      best = g;
      for (int r = tid; r < R; r += DUAL_THREADS) { best_pt[r] = al[r]; best_pt[R + r] = be[r]; }
    }
    const bool last = it == a.n_iter;
    const int what = (last ? 0 : DUAL_STEP) | (it == 0 && a.grad_alpha ? DUAL_GRAD : 0);
    if (!what) break;
    b1t *= 0.9; b2t *= 0.999;
    __syncthreads();
    dual_forward(a, b, tid, dual_lds, xs, what, 1.0 - b1t, 1.0 - b2t);
    if (last) break;
  }
  __syncthreads();
  for (int r = tid; r < R; r += DUAL_THREADS) { al[r] = best_pt[r]; be[r] = best_pt[R + r]; }
  __syncthreads();
  (void)dual_backward(a, b, tid, dual_lds, lam_ws, xs);
  dual_forward(a, b, tid, dual_lds, xs, DUAL_RECOVER, 1.0, 1.0);
  if (tid == 0) {
    a.bound[b] = best;
    if (a.lb32_prop) a.lb32_prop[b] = (float)best;
  }
}
