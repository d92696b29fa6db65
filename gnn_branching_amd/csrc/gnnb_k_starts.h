// gnnb_k_starts.h -- the upper bound from many starts: the restarts of the reference's get_upper_bound_pgd
// (plnn/conv_kwinter_gen.py:54-135: the LP point in slot 0, uniform points of the domain in the others) and of its sibling
// get_upper_bound_random (:20-52), on the device.  Between the two kernels here runs k_net_descend_tile<NS_TILE> (gnnb_k_net.h): the
// descent of every start, NS_TILE starts of one row per workgroup, each start's best point and value left in the workspace for the pick.
//
//   * k_net_starts          the start points of B rows: slot 0 = x0[b], slot r >= 1 a counter-based uniform point of the row's box.  No
//                           generator state: coordinate (r, m) of a row is a hash of the row's KEY and its own counter, and the key is
//                           seed + an integer sum over the row's x0 -- so a row's starts depend on its own x0, box and seed only, never on
//                           B, its index or what ran before.
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

#ifdef __HIPCC__      // (a plain C++ compiler takes the hash above alone: csrc/gnnb_replay_test.cpp)

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

struct NetPickArgs {
  const float* xb; const double* val;                   // (B, n_starts, N_0), (B, n_starts)
  int n_starts, N0;
  float* x_best; double* value; int32_t* start_index; double* start_value;      // (B, N_0), (B), null or (B), null or (B, n_starts)
};

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

#endif  // __HIPCC__
