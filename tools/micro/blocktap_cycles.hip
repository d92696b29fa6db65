// dev micro-benchmark (GPU box): the tap loop of ONE forward tile of edge 1 (cifar_base_kw: 3x32x32 -> 8x16x16, k 4, stride 2; a tile is
// 8 output channels x 2 positions, its union window 4 x 6 x 3 channels = 72 source rows of 64 floats) in two forms:
//   old    v_mfma_f32_16x16x4_f32: 20 k-steps x 4 M-tiles = 80 MFMAs of 32 cycles over the 80-slot padded union window
//          (gather_tile16 of gnnb_k_gather.h: one b128 per lane and k-step, the tap column and the row offset out of LDS)
//   block  v_mfma_f32_4x4x1_16b_f32: 16 blocks = channels 4b .. 4b+3 of one source row (lane e holds channel e: one dword per lane),
//          4 columns = 4 destination channels of ONE position; each position walks only its own 48 slots, 2 channel groups:
//          192 MFMAs of 8 cycles on four independent accumulators.  Taps: one ds_read_b128 per (position, group, window row) = per
//          4 MFMAs, the same four words in all 16 blocks (LDS broadcast).  <G0, G1>: groups issued for position 0 / 1 (dead groups
//          skipped: 2,2 = all 192 MFMAs; the mix draws 1 or 2 per position as ceil(Bin(8, 0.54) / 4) does, ~144 MFMAs per tile).
// Both with the source rows held in registers (the tap loop alone) and loaded from an L2-resident image as the product loads them, at two
// and four waves per SIMD on every CU, cycle counter and HIP events side by side; every case REPS times, median and spread printed.
// Then each form beside a wave of v_fma_f32 on the same SIMD (as mfma_valu_overlap.hip): does the vector wave get the freed cycles?
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -o tools/micro/blocktap_cycles tools/micro/blocktap_cycles.hip && tools/micro/blocktap_cycles
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>
typedef float f32x4 __attribute__((ext_vector_type(4)));

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); exit(1); } } while (0)

constexpr int SRC_W = 32, SRC_HW = 32 * 32, SRC_ROWS = 3 * SRC_HW;   // source layer: (c, y, x) -> row c * 1024 + y * 32 + x, 64 floats each
constexpr int NSAMPLES = 8;                                         // 8 x 768 KB of rows: L2 / MALL resident
constexpr int OLD_KSTEPS = 20;
constexpr int CM_FLOATS = OLD_KSTEPS * 64;                          // old form: tap column of (slot 4s+g, dst node i) at [s * 64 + lane]
constexpr int KVO_WORDS = OLD_KSTEPS * 4;                           // old form: byte offset of window slot from the window origin
constexpr int TAP_FLOATS = 4 * 12 * 4 * 4;                          // block form: [position * 2 + group][c * 4 + y][dst j][x 0..3]
constexpr int NMASK = 256;                                          // block form: (groups of position 0, of position 1) per tile
constexpr int LDS_FLOATS = CM_FLOATS + KVO_WORDS + TAP_FLOATS + NMASK;

// origin of tile t's window in the source image (interior tiles only: every row read is in range, see main())
__device__ __forceinline__ int tile_origin(int t) {
  const int y = (t >> 3) & 15, xp = t & 7;
  const int wy0 = min(2 * y, SRC_W - 4), wx0 = min(4 * xp, SRC_W - 6);
  return wy0 * SRC_W + wx0;
}

template <bool LOADS>
__device__ __forceinline__ void old_tile(f32x4 (&acc)[4], const float* cm, const unsigned* kvo, const float* rows, int origin, int lane) {
  const int g = lane >> 4, i = lane & 15;
  const float* base = rows + (long)origin * 64 + 4 * i;
  f32x4 cur[4], nxt[4];
  auto load = [&](f32x4 (&d)[4], int s0) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      if (LOADS) d[u] = *reinterpret_cast<const f32x4*>(base + (kvo[4 * (s0 + u) + g] >> 2));
      else d[u] = f32x4{0.25f + 0.001f * lane, -0.5f, 0.125f * (u + 1), 1.0f};
    }
  };
  auto mma = [&](const f32x4 (&v)[4], int s0) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const float b = cm[(s0 + u) * 64 + lane];
#pragma unroll
      for (int t = 0; t < 4; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(v[u][t], b, acc[t], 0, 0, 0);
    }
  };
  load(cur, 0);
#pragma unroll
  for (int s0 = 0; s0 < 16; s0 += 8) {
    load(nxt, s0 + 4);
    __builtin_amdgcn_sched_barrier(0);
    mma(cur, s0);
    __builtin_amdgcn_sched_barrier(0);
    load(cur, s0 + 8);
    __builtin_amdgcn_sched_barrier(0);
    mma(nxt, s0 + 4);
    __builtin_amdgcn_sched_barrier(0);
  }
  mma(cur, 16);
}

// one window row (c, y): six source rows x 0..5; position 0 takes x 0..3, position 1 x 2..5, each in x order; the two positions alternate,
// so an accumulator comes round every fourth MFMA
template <bool LOADS, int G0, int G1>
__device__ __forceinline__ void block_tile(f32x4 (&acc)[4], const float* tap, const float* rows, int origin, int lane) {
  const float* base = rows + (long)origin * 64 + lane;
  const f32x4* tp = reinterpret_cast<const f32x4*>(tap) + (lane & 3);
  struct Chunk { float r[6]; f32x4 t[4]; };           // the six rows and the taps of one window row, fetched one window row ahead
  Chunk cur, nxt;
  auto load = [&](Chunk& d, int cy) {
#pragma unroll
    for (int x = 0; x < 6; ++x) {
      if (LOADS) d.r[x] = base[((cy >> 2) * SRC_HW + (cy & 3) * SRC_W + x) * 64];
      else d.r[x] = 0.25f + 0.001f * lane + 0.125f * x;
    }
#pragma unroll
    for (int pg = 0; pg < 4; ++pg)
      if ((pg & 1) < ((pg >> 1) ? G1 : G0)) d.t[pg] = tp[(pg * 12 + cy) * 4];
  };
  auto mma = [&](const Chunk& c, int cy) {
#pragma unroll
    for (int x = 0; x < 4; ++x) {
#pragma unroll
      for (int pg = 0; pg < 4; ++pg)
        if ((pg & 1) < ((pg >> 1) ? G1 : G0)) acc[pg] = __builtin_amdgcn_mfma_f32_4x4x1f32(c.r[x + 2 * (pg >> 1)], c.t[pg][x], acc[pg], 0, 0, 0);
    }
  };
  load(cur, 0);
#pragma unroll
  for (int cy = 0; cy < 12; cy += 2) {
    load(nxt, cy + 1);
    __builtin_amdgcn_sched_barrier(0);
    mma(cur, cy);
    __builtin_amdgcn_sched_barrier(0);
    if (cy + 2 < 12) load(cur, cy + 2);
    __builtin_amdgcn_sched_barrier(0);
    mma(nxt, cy + 1);
    __builtin_amdgcn_sched_barrier(0);
  }
}

// FORM 0: old; 1: block, every group; 2: block, the groups of lds mask[tile]
template <int FORM, bool LOADS>
__device__ __forceinline__ void tile_loop(f32x4 (&acc)[4], const float* lds, const float* rows, int ntiles, int t0, int lane) {
  const float* cm = lds;
  const unsigned* kvo = reinterpret_cast<const unsigned*>(lds + CM_FLOATS);
  const float* tap = lds + CM_FLOATS + KVO_WORDS;
  const int* mask = reinterpret_cast<const int*>(lds + CM_FLOATS + KVO_WORDS + TAP_FLOATS);
  for (int t = t0; t < t0 + ntiles; ++t) {
    const int origin = tile_origin(t);
    if (FORM == 0) old_tile<LOADS>(acc, cm, kvo, rows, origin, lane);
    else if (FORM == 1) block_tile<LOADS, 2, 2>(acc, tap, rows, origin, lane);
    else {
      const int m = __builtin_amdgcn_readfirstlane(mask[t & (NMASK - 1)]);
      if (m == 0) block_tile<LOADS, 1, 1>(acc, tap, rows, origin, lane);
      else if (m == 1) block_tile<LOADS, 2, 1>(acc, tap, rows, origin, lane);
      else if (m == 2) block_tile<LOADS, 1, 2>(acc, tap, rows, origin, lane);
      else block_tile<LOADS, 2, 2>(acc, tap, rows, origin, lane);
    }
  }
}

__device__ __forceinline__ void stage(float* lds, const float* img) {
  for (int i = threadIdx.x; i < LDS_FLOATS; i += blockDim.x) lds[i] = img[i];
  __syncthreads();
}

template <int FORM, bool LOADS>
__global__ __launch_bounds__(1024) void k_tiles(const float* img, const float* rows, float* out, unsigned long long* cyc, int ntiles) {
  __shared__ __attribute__((aligned(16))) float lds[LDS_FLOATS];
  stage(lds, img);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  f32x4 acc[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) acc[q] = f32x4{0.f, 0.f, 0.f, 0.f};
  const float* r = rows + (long)(blockIdx.x % NSAMPLES) * SRC_ROWS * 64;
  const unsigned long long c0 = __builtin_readcyclecounter();
  tile_loop<FORM, LOADS>(acc, lds, r, ntiles, 16 * wave + blockIdx.x, lane);
  const unsigned long long c1 = __builtin_readcyclecounter();
  if (lane == 0) cyc[blockIdx.x * (blockDim.x >> 6) + wave] = c1 - c0;
  float s = 0.f;
#pragma unroll
  for (int q = 0; q < 4; ++q) s += acc[q][0] + acc[q][1] + acc[q][2] + acc[q][3];
  out[blockIdx.x * blockDim.x + threadIdx.x] = s;
}

// 512 threads per CU: waves 0-3 (one per SIMD) the tap loop, waves 4-7 (their SIMD partners) a v_fma_f32 loop; mode bit 0 / 1 enables them
template <int FORM>
__global__ __launch_bounds__(512) void k_beside(const float* img, const float* rows, float* out, unsigned long long* cyc, int ntiles, int n_valu, int mode) {
  __shared__ __attribute__((aligned(16))) float lds[LDS_FLOATS];
  stage(lds, img);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  f32x4 acc[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) acc[q] = f32x4{0.f, 0.f, 0.f, 0.f};
  float s = 0.f;
  const unsigned long long c0 = __builtin_readcyclecounter();
  if (wave < 4 && (mode & 1)) {
    tile_loop<FORM, false>(acc, lds, rows, ntiles, 16 * wave + blockIdx.x, lane);
#pragma unroll
    for (int q = 0; q < 4; ++q) s += acc[q][0] + acc[q][1] + acc[q][2] + acc[q][3];
  }
  if (wave >= 4 && (mode & 2)) {
    float v0 = lane, v1 = lane + 1, v2 = lane + 2, v3 = lane + 3, v4 = lane + 4, v5 = lane + 5, v6 = lane + 6, v7 = lane + 7;
    const float c = 1.0001f, d = 0.5f;
    for (int i = 0; i < n_valu; i += 8) {
      v0 = __builtin_fmaf(v0, c, d); v1 = __builtin_fmaf(v1, c, d); v2 = __builtin_fmaf(v2, c, d); v3 = __builtin_fmaf(v3, c, d);
      v4 = __builtin_fmaf(v4, c, d); v5 = __builtin_fmaf(v5, c, d); v6 = __builtin_fmaf(v6, c, d); v7 = __builtin_fmaf(v7, c, d);
      asm volatile("" : "+v"(v0), "+v"(v1), "+v"(v2), "+v"(v3), "+v"(v4), "+v"(v5), "+v"(v6), "+v"(v7));
    }
    s = v0 + v1 + v2 + v3 + v4 + v5 + v6 + v7;
  }
  const unsigned long long c1 = __builtin_readcyclecounter();
  if (lane == 0) cyc[blockIdx.x * 8 + wave] = c1 - c0;
  out[blockIdx.x * blockDim.x + threadIdx.x] = s;
}

static const int NWG = 256, REPS = 7;
static float *d_img, *d_rows, *d_out;
static unsigned long long* d_cyc;

struct Stat { double med, spread; };   // spread: (max - min) / median over the REPS runs
static Stat stat(std::vector<double> v) {
  std::sort(v.begin(), v.end());
  return {v[v.size() / 2], (v.back() - v.front()) / v[v.size() / 2]};
}

struct Res { Stat us, ticks; };
template <int FORM, bool LOADS>
static Res run_tiles(int waves, int ntiles) {
  hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
  std::vector<double> us, tk;
  std::vector<unsigned long long> h(NWG * waves);
  k_tiles<FORM, LOADS><<<NWG, waves * 64>>>(d_img, d_rows, d_out, d_cyc, ntiles);      // warm-up
  for (int r = 0; r < REPS; ++r) {
    CK(hipEventRecord(e0));
    k_tiles<FORM, LOADS><<<NWG, waves * 64>>>(d_img, d_rows, d_out, d_cyc, ntiles);
    CK(hipEventRecord(e1));
    CK(hipDeviceSynchronize());
    float ms = 0; CK(hipEventElapsedTime(&ms, e0, e1));
    CK(hipMemcpy(h.data(), d_cyc, h.size() * 8, hipMemcpyDeviceToHost));
    double sum = 0;
    for (auto v : h) sum += (double)v;
    us.push_back(1e3 * ms);
    tk.push_back(sum / h.size() / ntiles);
  }
  CK(hipEventDestroy(e0)); CK(hipEventDestroy(e1));
  return {stat(us), stat(tk)};
}

static const char* form_name(int f) { return f == 0 ? "old 16x16x4, 80 MFMAs" : f == 1 ? "block 4x4x1, 192 MFMAs" : "block 4x4x1, live mix ~144"; }

template <bool LOADS>
static void table(int ntiles) {
  printf("\n== tap loop, %s; %d tiles per wave, %d CUs, %d runs each ==\n", LOADS ? "rows loaded (L2-resident image)" : "rows in registers", ntiles, NWG, REPS);
  for (int waves : {8, 16}) {
    const Res r[3] = {run_tiles<0, LOADS>(waves, ntiles), run_tiles<1, LOADS>(waves, ntiles), run_tiles<2, LOADS>(waves, ntiles)};
    for (int f = 0; f < 3; ++f) {
      // ns per tile and SIMD: wall / (tiles per wave x waves per SIMD); x 2.4 GHz ~ pipe cycles a tile holds its SIMD
      const double ns = 1e3 * r[f].us.med / ntiles / (waves / 4);
      printf("%-28s %d waves/SIMD: kernel %9.1f us (spread %.2f %%)  %7.1f ns per tile and SIMD  %8.0f ticks per tile and wave (spread %.2f %%)", form_name(f),
             waves / 4, r[f].us.med, 100 * r[f].us.spread, ns, r[f].ticks.med, 100 * r[f].ticks.spread);
      if (f) {
        const double ratio = r[f].us.med / r[0].us.med, sp = std::max(r[f].us.spread, r[0].us.spread);
        printf("  wall / old = %.3f  gain %.1f %% vs 3 x spread %.1f %% -> %s", ratio, 100 * (1 - ratio), 300 * sp, (1 - ratio) > 3 * sp ? "FASTER" : "not faster");
      }
      printf("\n");
    }
  }
}

template <int FORM>
static void beside(int ntiles, int n_valu) {
  std::vector<unsigned long long> h(NWG * 8);
  double tap[4] = {0, 0, 0, 0}, val[4] = {0, 0, 0, 0}, us[4] = {0, 0, 0, 0};
  hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
  for (int mode = 1; mode <= 3; ++mode) {
    std::vector<double> a, b, w;
    k_beside<FORM><<<NWG, 512>>>(d_img, d_rows, d_out, d_cyc, ntiles, n_valu, mode);
    for (int r = 0; r < REPS; ++r) {
      CK(hipEventRecord(e0));
      k_beside<FORM><<<NWG, 512>>>(d_img, d_rows, d_out, d_cyc, ntiles, n_valu, mode);
      CK(hipEventRecord(e1));
      CK(hipDeviceSynchronize());
      float ms = 0; CK(hipEventElapsedTime(&ms, e0, e1));
      CK(hipMemcpy(h.data(), d_cyc, h.size() * 8, hipMemcpyDeviceToHost));
      double sa = 0, sb = 0;
      for (int g = 0; g < NWG; ++g)
        for (int q = 0; q < 4; ++q) { sa += (double)h[g * 8 + q]; sb += (double)h[g * 8 + 4 + q]; }
      a.push_back(sa / (4 * NWG)); b.push_back(sb / (4 * NWG)); w.push_back(1e3 * ms);
    }
    tap[mode] = stat(a).med; val[mode] = stat(b).med; us[mode] = stat(w).med;
  }
  CK(hipEventDestroy(e0)); CK(hipEventDestroy(e1));
  printf("%-28s tap wave alone %9.0f ticks (%.1f us)   v_fma wave alone %9.0f ticks (%.1f us)   together: tap %9.0f, v_fma %9.0f ticks (%.1f us)"
         "   together / (sum of alone) = %.3f, / max = %.3f\n",
         form_name(FORM), tap[1], us[1], val[2], us[2], tap[3], val[3], us[3], us[3] / (us[1] + us[2]), us[3] / std::max(us[1], us[2]));
}

int main() {
  std::vector<float> img(LDS_FLOATS), rows((size_t)NSAMPLES * SRC_ROWS * 64);
  srand(1);
  auto rnd = [] { return ((rand() % 2001) - 1000) * 1e-3f; };      // random data: all-zero operands let the chip clock higher
  // old form: slot q = 4s + g of the union window, (c, y, x) = (q / 24, q / 6 % 4, q % 6); slots 72..79 are padding (tap 0, offset 0).
  // dst node i = (out channel i >> 1 ... ) is immaterial here; position i & 1 sees columns 2 (i & 1) .. + 3: the other taps are ZERO, as in the product
  unsigned* kvo = reinterpret_cast<unsigned*>(img.data() + CM_FLOATS);
  for (int q = 0; q < 80; ++q) {
    const int c = q / 24, y = q / 6 % 4, x = q % 6, s = q >> 2, g = q & 3;
    kvo[q] = q < 72 ? (unsigned)(c * SRC_HW + y * SRC_W + x) * 256u : 0u;
    for (int i = 0; i < 16; ++i) {
      const int p = i & 1;
      img[s * 64 + g * 16 + i] = (q < 72 && x >= 2 * p && x < 2 * p + 4) ? 0.1f * rnd() : 0.0f;
    }
  }
  for (int i = 0; i < TAP_FLOATS; ++i) img[CM_FLOATS + KVO_WORDS + i] = 0.1f * rnd();
  int* mask = reinterpret_cast<int*>(img.data() + CM_FLOATS + KVO_WORDS + TAP_FLOATS);
  double mean_groups = 0;
  for (int t = 0; t < NMASK; ++t) {       // groups of a position: ceil(n / 4), n ~ Bin(8, 0.54) -> two groups with probability 0.452
    const int g0 = (rand() % 1000) < 452, g1 = (rand() % 1000) < 452;
    mask[t] = g0 | (g1 << 1);
    mean_groups += 2 + g0 + g1;
  }
  for (auto& v : rows) v = rnd();
  // every load stays inside one sample's image: the largest row read is (2, 28 + 3, 26 + 5) = 3071 < SRC_ROWS (tile_origin clamps)
  CK(hipMalloc(&d_img, img.size() * 4)); CK(hipMalloc(&d_rows, rows.size() * 4)); CK(hipMalloc(&d_out, (size_t)NWG * 1024 * 4)); CK(hipMalloc(&d_cyc, NWG * 16 * 8));
  CK(hipMemcpy(d_img, img.data(), img.size() * 4, hipMemcpyHostToDevice));
  CK(hipMemcpy(d_rows, rows.data(), rows.size() * 4, hipMemcpyHostToDevice));
  printf("blocktap_cycles: one edge-1 forward tile's tap loop, old 16x16x4 form vs 4x4x1 16-block form; live mix issues %.1f of 192 MFMAs per tile\n",
         48.0 * mean_groups / NMASK);
  printf("issue model: old 80 x 32 = 2560 cycles; block 192 x 8 = 1536 (0.60); live mix ~144 x 8 = 1150 (0.45)\n");
  table<false>(1000);
  table<true>(1000);
  printf("\n== beside a v_fma_f32 wave on the same SIMD (rows in registers; 400 tiles, 256K v_fma_f32 per vector wave) ==\n");
  beside<0>(400, 1 << 18);
  beside<1>(400, 1 << 18);
  beside<2>(400, 1 << 18);
  CK(hipFree(d_img)); CK(hipFree(d_rows)); CK(hipFree(d_out)); CK(hipFree(d_cyc));
  return 0;
}
