// gnnb.hip -- MI355X (gfx950 / CDNA4) GNN branching-score forward pass: HIP kernels + C-ABI.
//
// What runs here is the reference's graphnet/graph_conv.py (EmbedLayerUpdate.forward :77-388,
// ComputeFinalScore.forward :442-470), the argmax of graphnet/graph_score.py :41-47 and the BaBSR heuristic of
// plnn/kw_score_conv.py :41-113, for a batch of B subproblems, re-designed for CDNA4 (DESIGN.md sections 3-5):
//
//   * embeddings mu[k] live in HBM as (B, N_k, 64) fp32, one 256-B row per node;
//   * every node MLP is a chain of exact-fp32 MFMAs (v_mfma_f32_32x32x2_f32) run TRANSPOSED: weights are the A operand
//     (staged once per workgroup in LDS, pre-permuted on the host, gnnb_pack.h), the 32 nodes of a tile sit on the lanes,
//     and the accumulators of one layer are the B operands of the next -- no LDS round trip between layers;
//   * node-feature-only sub-chains do not depend on the embeddings: evaluated ONCE per forward (k_pre) and folded
//     into a cached 64-vector per ambiguous node; linear layers that meet are pre-multiplied on the host; every producer's
//     last Linear is deferred into its consumers ("deferred projection", gnnb_pack.h);
//   * node classes (live / ambiguous / scored) are compacted once per forward (k_classify) and the node MLPs run over
//     the lists only;
//   * conv / conv-transpose message passing is a dense local block per tile on the MFMA (k_gather, k_gather16,
//     k_gather_input_update), Linear edges and everything above the last conv layer run per sample out of LDS (k_top);
//   * provably dead work of the reference is not executed: the `ratio` chain (:214-216,228,243,356) and the last
//     round's input-layer update (:360-385), whose result nothing reads.
//
// One translation unit: gnnb_dev.h (fragments, GEMM blocks, tile maps), gnnb_k_mlp.h (setup + node-MLP kernels),
// gnnb_k_gather.h (conv-edge message passing + score head), gnnb_k_fusedq.h (gather + node update in one kernel), gnnb_k_edges.h (other edges, k_top), gnnb_k_misc.h (k_livesum,
// k_babsr, k_gather_scored), gnnb_k_kw.h (Wong-Kolter bounds, gnnb_kw_bounds), gnnb_k_dual.h (dual ascent, gnnb_dual_ascent), gnnb_k_net.h (the fp64 walk of the
// bound network, gnnb_net_eval / gnnb_net_descend / gnnb_net_descend_starts), gnnb_k_frontier.h (the steps of a BaB round on a
// device-resident frontier, gnnb_frontier_*), gnnb_k_starts.h (start points and the pick), gnnb_train.h (online learning: the tape; its kernels in gnnb_k_train.h, the step and its entry
// points in gnnb_step.h) are included below; this file
// holds the host side and the C-ABI.
//
// gfx950 only.  No HIP call at load time.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include <thread>
#include <unistd.h>
#include <sched.h>
#include <atomic>
#include <condition_variable>
#include <functional>
#include <memory>
#include <mutex>

#include "../../include/gnnb.h"
#include "gnnb_pack.h"
#include "gnnb_mem.h"
#include "gnnb_train.h"

using namespace gnnb;

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

#include "gnnb_dev.h"
#include "gnnb_k_mlp.h"
#include "gnnb_k_gather.h"
#include "gnnb_k_fusedq.h"
#include "gnnb_k_edges.h"
#include "gnnb_k_misc.h"
#include "gnnb_k_kw.h"
#include "gnnb_k_dual.h"
#include "gnnb_k_tighten.h"
#include "gnnb_k_net.h"
#include "gnnb_k_frontier.h"
#include "gnnb_k_starts.h"
#include "gnnb_k_strong.h"
#include "gnnb_k_repack.h"
#include "gnnb_k_replay.h"

#define N_PACKS 14   // == PK_COUNT
enum { PK_EMBED, PK_PRE_FWD, PK_PRE_BWD, PK_PRE_INP, PK_PROP, PK_UPD_FWD_E, PK_UPD_FWD_I, PK_UPD_FWD_F, PK_UPD_BWD, PK_UPD_BWD_B,
       PK_UPD_INP, PK_POST_INP, PK_SCORE_B, PK_SCORE_F, PK_COUNT };
static_assert(PK_COUNT == N_PACKS, "pack table");
static_assert(kMaxReluLayers == MAXL && kMaxLayerNodes == LIVESUM_MAXSRC && kDenseChunk == DENSE_CH, "gnnb_pack.h: the kernels' limits");

// ------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------
static thread_local std::string g_err;
static int fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_err = buf;
  fprintf(stderr, "[gnnb] error: %s\n", buf);   // the BaB harness swallows exceptions (bab_mip.py:73-76): log first
  return code;
}
#define HIPCHK(x)                                                                         \
  do {                                                                                    \
    hipError_t e_ = (x);                                                                  \
    if (e_ != hipSuccess) return fail(GNNB_E_HIP, "%s: %s (%s:%d)", #x, hipGetErrorString(e_), __FILE__, __LINE__); \
  } while (0)

enum ProfClass {
  PC_EMBED, PC_PRE, PC_PRE_INP, PC_CONV_FWD, PC_CONVT_BWD, PC_DENSE_AGG, PC_PROP_FWD,
  PC_NODE_UPDATE, PC_INPUT_UPDATE, PC_SCORE, PC_ARGMAX, PC_GATHER, PC_GATHER_INPUT, PC_CLASSIFY, PC_LIVESUM, PC_TOP, PC_GATHER_UPDATE,
  PC_KW_FIRST, PC_KW_LAYER, PC_KW_FLAG, PC_DUAL,
  PC_FR_GATHER, PC_FR_EXPAND, PC_NET_EVAL, PC_FR_RESOLVE, PC_FR_DECIDE, PC_FR_STORE, PC_FR_PICK_JOBS, PC_FR_ROWS_JOBS, PC_FR_DECIDE_JOBS,
  PC_FR_CANDIDATES, PC_FR_FALLBACK, PC_FR_CHOOSE, PC_FR_CHOOSE_COPY, PC_FR_FALLBACK_JOBS, PC_FR_SELECT_JOBS, PC_FR_ROWS_SEL, PC_FR_CHOOSE_JOBS,
  PC_FR_LEARN, PC_TROWS_GATHER, PC_NET_DESCEND, PC_FR_WITNESS, PC_FR_WITNESS_JOBS,
  PC_NET_STARTS, PC_NET_DESCEND_TILE, PC_NET_STARTS_PICK, PC_FR_BABSR_DECIDE, PC_FR_BABSR_DECIDE_JOBS,
  PC_STRONG_COUNT, PC_STRONG_COMPACT, PC_STRONG_PICK, PC_COUNT
};
static const char* kProfNames[PC_COUNT] = {
    "k_embed", "k_pre", "k_pre_inp", "k_conv_fwd", "k_convT_bwd", "k_dense_agg", "k_prop",
    "k_node_update", "k_input_update", "k_score", "k_argmax", "k_gather", "k_gather_input_update", "k_classify", "k_livesum", "k_top", "k_gather_update",
    "k_kw_first", "k_kw_layer", "k_kw_flag", "k_dual_ascent",
    "k_frontier_gather", "k_frontier_expand", "k_net_eval", "k_frontier_resolve", "k_frontier_decide", "k_frontier_store",
    "k_frontier_pick_jobs", "k_frontier_rows_jobs", "k_frontier_decide_jobs",
    "k_frontier_candidates", "k_frontier_fallback", "k_frontier_choose", "k_frontier_choose_copy",
    "k_frontier_fallback_jobs", "k_frontier_select_jobs", "k_frontier_rows_sel", "k_frontier_choose_jobs",
    "k_frontier_learn", "k_trows_gather", "k_net_descend", "k_frontier_witness", "k_frontier_witness_jobs",
    "k_net_starts", "k_net_descend_tile", "k_net_starts_pick", "k_frontier_babsr_decide", "k_frontier_babsr_decide_jobs",
    "k_strong_count", "k_strong_compact", "k_strong_pick"};

struct DevEdge : DenseGeom {
  DevBuf<float> w_fwd, w_bwd, bias;   // conv: tap-major copies; linear: W^T / W, zero-padded (gnnb_pack.h dense_operands)
};

struct DevGather {          // one conv edge in one direction, as MFMA gather tables on the device
  bool ok = false;
  GatherGeom g;
  DevBuf<float> cmat;
  DevBuf<int> koff, ttab;
};

// Everything gnnb_bind_network produces.  A bind builds a fresh one and move-assigns it into the handle on success; dropping it
// releases the network's device memory.
struct BoundNet : LayerGraph {
  bool bound = false;
  std::vector<DevEdge> dev;
  std::vector<DevGather> gf, gb;   // gf[k]: edge k forward (dst = layer k); gb[k]: edge k transposed (dst = layer k-1)
  std::vector<DevBuf<double>> kw_w, kw_b;  // fp64 copies of edge k's weights (torch layout) and bias for the fp64 kernels, k = 1..L
  KwNet kw_net{};                   // the bound network as gnnb_kw_bounds / gnnb_dual_ascent pass it to their kernels
  bool top_ok = false;              // the network allows k_top (option `top`)
  int zero_tap[3] = {0, 0, 0};      // {k, y, x}: inner conv edge k leaves pixel (y, x) of layer k-1 without a tap (k = 0: none)
  DevBuf<float> d_s1;               // (N_1) bias sums of edge 1 forward over the (all live) input layer: sum of the weights that reach each node
  std::vector<DevBuf<float>> edge_w;   // torch-layout weights of the edges for the trainer, made by the first gnnb_online_step
};

// Host helper threads of a handle, created by the first call that wants them (work_pool below) and joined by gnnb_destroy: creating
// and joining threads per call cost 0.25 ms of a 0.65-ms pack.  Idle workers sleep on a condition variable.  (A handle is created in the
// process that uses it -- the BaB harness forks first, bab_mip.py:244-249 -- so no thread ever has to survive a fork.)
struct WorkPool {
  std::vector<std::thread> th;
  std::mutex m;
  std::condition_variable cv, done_cv;
  const std::function<void()>* job = nullptr;
  long gen = 0;
  int busy = 0;
  bool stop = false;
  pid_t owner = getpid();             // a forked child inherits the object but not the threads: it makes a pool of its own (work_pool)
  explicit WorkPool(int n) {
    for (int i = 0; i < n; ++i)
      th.emplace_back([this] {
        long seen = 0;
        for (;;) {
          const std::function<void()>* f;
          {
            std::unique_lock<std::mutex> lk(m);
            cv.wait(lk, [&] { return stop || gen != seen; });
            if (stop) return;
            seen = gen;
            f = job;
          }
          (*f)();
          {
            std::lock_guard<std::mutex> lk(m);
            if (--busy == 0) done_cv.notify_one();
          }
        }
      });
  }
  std::mutex callers;                 // one run() at a time: `job` points into the caller's frame (two pipelines on one engine, ctypes drops the GIL)
  void run(const std::function<void()>& f) {      // f on every worker and on the caller; returns when all are done
    std::lock_guard<std::mutex> one(callers);
    {
      std::lock_guard<std::mutex> lk(m);
      job = &f; ++gen; busy = (int)th.size();
    }
    cv.notify_all();
    f();
    std::unique_lock<std::mutex> lk(m);
    done_cv.wait(lk, [&] { return busy == 0; });
  }
  ~WorkPool() {
    {
      std::lock_guard<std::mutex> lk(m);
      stop = true;
    }
    cv.notify_all();
    for (auto& t : th) t.join();
  }
};

struct gnnb_handle : BoundNet {
  WorkPool* work_pool = nullptr;      // see WorkPool; made and replaced by work_pool(h) alone, under pool_mutex
  std::mutex pool_mutex;
  int T = 2, p = 64, device = 0, n_cu = 256;
  bool use_gather = true;       // MFMA gather for conv edges (false: VALU gather kernels)
  // (k_node_update: 12 waves per workgroup = 3 per SIMD with the bf16x3 blocks (142-152 VGPRs, no scratch); the fp32-MFMA-only
  // form (option bf3 = 0) needs 167-181 VGPRs and runs 8 waves per workgroup)
  bool dense_lds = true;        // Linear edges: one workgroup per sample with the source rows in LDS (false: per-tile kernel)
  bool bf3 = true;              // node update: 64x64 blocks on the bf16 matrix rate with three-piece operands (fp32 accuracy)
  bool embed_fuse = true;       // round 0: the first forward gather computes the input embedding itself (no k_embed, no mu[0] rows)
  int fuse = 1;                 // conv half-passes as ONE kernel (k_gather_update_q: the aggregate never reaches HBM) wherever that kernel
                                // exists (measured faster at every batch size and on all three networks: base B = 256 0.975 vs 1.014 ms,
                                // deep B = 1024 6.59 vs 7.31 ms, B = 1 0.344 vs 0.359 ms); fuse = 0: always two kernels.  Both forms
                                // compute the same arithmetic per node -- bit-identical results -- so this is a pure scheduling choice.
  bool use_top = true;          // fuse the top of the network (last Linear edge, last ReLU layer, property node) into k_top (where BoundNet::top_ok)
  int clspre_max_b = 1;         // option clspre_max_b: batches up to it classify and run the hoisted feature chains in one launch (k_classify_pre);
                                // measured (base, us): B = 1 27.5 vs 7.6 + 22.1, B = 2 34.0 vs 30.0, B = 8 42.5 vs 31.8 -- a block's share of
                                // the ambiguous nodes is uneven, so beyond one subproblem the two kernels' even dealing wins
  int tail_max_b = 1 << 30;     // option tail_max_b: batches up to it end in k_scored_tail (scored gather + restricted update + score head in one launch); 0: three kernels
  bool top_fuse_upd = true;     // option top_fuse_upd = 0: the backward node update of layer L-1 as its own launch behind k_top (it runs inside k_top otherwise)
  int top_split_max = 4;        // option top_split: 4 (default) = four workgroups per sample while B <= n_cu / 4, two while B <= n_cu / 2; 2 = two at most; 1 = never
  Packs packs;
  std::vector<float> blob;      // the GNN parameters as handed to gnnb_create / gnnb_set_weights / left by gnnb_online_step
  std::unique_ptr<gnnb_train::Trainer> trainer;     // online learning (gnnb_online_create)
  DevBuf<float> pack_block;     // the weight packs, one block ...
  float* d_pack[N_PACKS] = {nullptr};      // ... and where pack i starts in it (load_weights)
  // the device pack builder (gnnb_k_repack.h; made with the trainer): fold scratch and segment table; repack_mode 1: the packs follow
  // the trainer's d_w on the stream and `blob` is refreshed from it on demand (fresh_blob)
  int repack_mode = 0;
  bool blob_stale = false;
  DevBuf<float> repack_scr;
  DevBuf<RepackSeg> repack_segs;
  int repack_nseg = 0, repack_nblocks = 0;
  DevBuf<int> replay_slot;      // gnnb_replay_push: the ring slot of every listed row (k_replay_rank writes it, k_replay_store reads it)
  DevBuf<float> d_zero;         // 64 zero floats: where masked gather loads point
  // List counters of a forward (64 ints) live HERE, not in the caller's workspace: a control block per workspace address (CTL_SLOTS
  // of them, least recently used replaced), zero whenever no forward is running on it -- the last workgroup of k_score, the last
  // kernel of a forward and the last reader of the counters, puts them back to zero.  So no launch has to zero them first
  // (k_reset is gone), and what the caller's workspace holds between calls does not matter.
  PinnedBuf<float> pack_stage;  // pinned staging of the weight packs (load_weights)
  DevBuf<int> d_ctl;
  const void* ctl_ws[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  unsigned long ctl_age[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  unsigned long ctl_clock = 0;
  // gnnb_forward_host: pinned staging of the host inputs, their device image, workspace and outputs (grown on demand)
  PinnedBuf<float> hs_pinned, hs_out_pinned;
  DevBuf<float> hs_dev, hs_scores;
  DevBuf<char> hs_ws;
  DevBuf<int32_t> hs_dec;
  int last_proj[MAXL + 2];      // per graph layer: which Linear (LayerId) the rows of mu[k] written by the LAST forward still have to
                                // go through (-1: final) -- the "deferred projection" of gnnb_pack.h; inspection only (gnnb_mu_projection),
                                // gnnb_forward itself keeps this state on its stack
  int halfpass_limit = 0;
  bool prof = false;
  struct Ev { int cls; hipEvent_t a, b; };
  std::vector<Ev> pending;
  struct Tr { int cls; float ms; };
  std::vector<Tr> trace;          // per-launch record of what gnnb_profile_read resolved (gnnb_profile_trace)
  std::vector<hipEvent_t> pool;
  double prof_ms[PC_COUNT] = {0};
  int64_t prof_n[PC_COUNT] = {0};
  hipStream_t prof_stream = nullptr;
};


// (re)build the operand packs of the scorer from a parameter blob and put them on the device
static int load_weights(gnnb_t* h, const float* w_blob, hipStream_t st) {
  h->blob.assign(w_blob, w_blob + blob_floats());
  build_packs(h->blob.data(), h->packs);
  const std::vector<float>* pv[N_PACKS] = {&h->packs.embed, &h->packs.pre_fwd, &h->packs.pre_bwd, &h->packs.pre_inp, &h->packs.prop,
                                           &h->packs.upd_fwd_e, &h->packs.upd_fwd_i, &h->packs.upd_fwd_f, &h->packs.upd_bwd,
                                           &h->packs.upd_bwd_b, &h->packs.upd_inp, &h->packs.post_inp, &h->packs.score_b,
                                           &h->packs.score_f};
  // the packs go through ONE pinned staging buffer: 14 copies out of pageable memory were each staged synchronously by the
  // runtime (0.3 ms of the 1.4 ms this call took behind every online-learning step)
  size_t total = 0;
  for (int i = 0; i < N_PACKS; ++i) total += (pv[i]->size() + 63) & ~(size_t)63;
  for (int i = 0; i < N_PACKS; ++i)
    if (pv[i]->size() != (size_t)kPackFloats[i]) return fail(GNNB_E_INVALID, "load_weights: pack %d has %zu floats, kPackFloats says %d", i, pv[i]->size(), kPackFloats[i]);
  h->blob_stale = false;
  HIPCHK(h->pack_stage.grow(total));
  if (!h->pack_block.get()) {             // one device block, pack i at the offset it has in the staging buffer: one copy per call
    HIPCHK(h->pack_block.alloc(total));
    size_t o = 0;
    for (int i = 0; i < N_PACKS; ++i) { h->d_pack[i] = h->pack_block.get() + o; o += (pv[i]->size() + 63) & ~(size_t)63; }
  }
  size_t off = 0;
  for (int i = 0; i < N_PACKS; ++i) {
    std::memcpy(h->pack_stage.get() + off, pv[i]->data(), pv[i]->size() * sizeof(float));
    off += (pv[i]->size() + 63) & ~(size_t)63;
  }
  HIPCHK(hipMemcpyAsync(h->pack_block.get(), h->pack_stage.get(), total * sizeof(float), hipMemcpyHostToDevice, st));
  HIPCHK(hipStreamSynchronize(st));       // the staging buffer is reused by the next call
  return 0;
}

extern "C" int gnnb_abi_version(void) { return GNNB_ABI_VERSION; }
#ifndef GNNB_SRC_HASH
#define GNNB_SRC_HASH "unhashed-build------------------"
#endif
// the hash of the sources this binary was compiled from (gnn_branching_amd/_lib.py source_hash): the loader refuses a library
// whose id differs from the tree's, the build skips one whose id matches (mtimes are not trusted: *.so ships outside git)
static const char g_build_id[] = "GNNB_BUILD_ID:" GNNB_SRC_HASH;
extern "C" const char* gnnb_build_id(void) { return g_build_id + 14; }
extern "C" const char* gnnb_last_error(void) { return g_err.c_str(); }


// ---- handle options (include/gnnb.h gnnb_set_option) ---------------------------------------------------------------------------------
// The shipped library reads NO environment variable: every switch a caller, a test or bench.py can flip goes through this table.  Each
// option selects between implementations that compute the same scores (bit-identical unless the comment says otherwise), so the parity
// tests use them as independent implementations of one another (INTEGRATION.md lists the test of each).
struct OptDesc { const char* name; int lo, hi; bool before_bind; };
static const OptDesc kOptions[] = {
    {"bf3", 0, 1, false},             // 1: 64x64 blocks on the bf16 matrix rate with three-piece operands; 0: every block exact fp32 MFMA (and no k_top)
    {"fuse", 0, 1, false},            // 1: a conv half-pass is ONE kernel (k_gather_update_q); 0: k_gather + k_node_update
    {"top", 0, 1, false},             // 1: the top of the network in k_top; 0: separate kernels (fp32 MFMA edges)
    {"gather", 0, 1, true},           // 1: MFMA gathers for conv edges; 0: the VALU conv kernels + flat node update
    {"embed_fuse", 0, 1, false},      // 1: round 0's input embedding computed inside the first gather; 0: k_embed writes the rows
    {"dense_lds", 0, 1, true},        // 1: Linear edges one workgroup per sample out of LDS; 0: the per-tile dense kernel (the fallback of wide layers)
    {"tail_max_b", 0, 1 << 30, false},    // batches up to it end in k_scored_tail; 0: k_gather_scored + k_node_update + k_score
    {"top_split", 1, 4, false},       // most workgroups k_top spreads one sample over (1, 2 or 4); 1 = never wait for a partner workgroup
    {"top_fuse_upd", 0, 1, false},    // 1: the backward update of layer L-1 inside k_top; 0: its own launch behind it
    {"clspre_max_b", 0, 1 << 30, false},  // batches up to it classify and run the hoisted feature chains in one launch (k_classify_pre)
};
static int* opt_field(gnnb_t* h, int i, bool** bf) {
  *bf = nullptr;
  switch (i) {
    case 0: *bf = &h->bf3; return nullptr;
    case 1: return &h->fuse;
    case 2: *bf = &h->use_top; return nullptr;
    case 3: *bf = &h->use_gather; return nullptr;
    case 4: *bf = &h->embed_fuse; return nullptr;
    case 5: *bf = &h->dense_lds; return nullptr;
    case 6: return &h->tail_max_b;
    case 7: return &h->top_split_max;
    case 8: *bf = &h->top_fuse_upd; return nullptr;
    default: return &h->clspre_max_b;
  }
}
static int opt_index(const char* name) {
  if (!name) return -1;
  for (int i = 0; i < (int)(sizeof kOptions / sizeof kOptions[0]); ++i)
    if (!strcmp(name, kOptions[i].name)) return i;
  return -1;
}
extern "C" int gnnb_option_count(void) { return (int)(sizeof kOptions / sizeof kOptions[0]); }
extern "C" const char* gnnb_option_name(int i) { return i >= 0 && i < gnnb_option_count() ? kOptions[i].name : ""; }
extern "C" int gnnb_set_option(gnnb_t* h, const char* name, int value) {
  if (!h) return fail(GNNB_E_INVALID, "gnnb_set_option: null handle");
  const int i = opt_index(name);
  if (i < 0) return fail(GNNB_E_INVALID, "gnnb_set_option: unknown option '%s'", name ? name : "(null)");
  const OptDesc& d = kOptions[i];
  if (value < d.lo || value > d.hi) return fail(GNNB_E_INVALID, "gnnb_set_option: %s = %d outside [%d, %d]", d.name, value, d.lo, d.hi);
  if (d.before_bind && h->bound) return fail(GNNB_E_STATE, "gnnb_set_option: %s must be set before gnnb_bind_network (it shapes the tables built there)", d.name);
  bool* bf = nullptr;
  int* f = opt_field(h, i, &bf);
  if (bf) *bf = value != 0;
  else *f = (i == 7) ? (value >= 4 ? 4 : (value >= 2 ? 2 : 1)) : value;
  return GNNB_OK;
}
extern "C" int gnnb_get_option(const gnnb_t* h, const char* name, int* value) {
  if (!h || !value) return fail(GNNB_E_INVALID, "gnnb_get_option: null argument");
  const int i = opt_index(name);
  if (i < 0) return fail(GNNB_E_INVALID, "gnnb_get_option: unknown option '%s'", name ? name : "(null)");
  bool* bf = nullptr;
  int* f = opt_field(const_cast<gnnb_t*>(h), i, &bf);
  *value = bf ? (*bf ? 1 : 0) : *f;
  return GNNB_OK;
}

struct LdsAttr {      // a kernel and the dynamic LDS it may be launched with
  const void* fn; size_t bytes;
  template <class F> LdsAttr(F* f, size_t b) : fn((const void*)f), bytes(b) {}
};

extern "C" int gnnb_create(gnnb_t** out, const float* w_blob, size_t n_floats, int T, int p) {
  if (!out || !w_blob) return fail(GNNB_E_INVALID, "gnnb_create: null argument");
  if (p != P) return fail(GNNB_E_INVALID, "gnnb_create: embedding size %d unsupported (kernels are built for p=64)", p);
  if (T < 1 || T > 16) return fail(GNNB_E_INVALID, "gnnb_create: T=%d out of range", T);
  if (n_floats != blob_floats()) return fail(GNNB_E_INVALID, "gnnb_create: weight blob has %zu floats, expected %zu", n_floats, blob_floats());
  int ndev = 0;
  hipError_t e = hipGetDeviceCount(&ndev);
  if (e != hipSuccess || ndev == 0) return fail(GNNB_E_HIP, "gnnb_create: no HIP device (%s)", hipGetErrorString(e));
  std::unique_ptr<gnnb_handle> h(new gnnb_handle());      // (a failure below releases it and what it holds)
  h->T = T;
  h->p = p;
  HIPCHK(hipGetDevice(&h->device));
  hipDeviceProp_t prop;
  HIPCHK(hipGetDeviceProperties(&prop, h->device));
  h->n_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
  if (int rc = load_weights(h.get(), w_blob, nullptr)) return rc;
  HIPCHK(h->d_zero.alloc(256));
  HIPCHK(hipMemset(h->d_zero.get(), 0, 256 * sizeof(float)));
  HIPCHK(h->d_ctl.alloc(8 * 64));
  HIPCHK(hipMemset(h->d_ctl.get(), 0, 8 * 64 * sizeof(int)));
  // > 64 KiB of dynamic LDS needs the attribute
  constexpr size_t kUpd = (PackUpd::FLOATS + 4096) * 4, kUpd3 = (PackUpdL3::FLOATS + 6144) * 4, k128 = 128 * 1024, k160 = 160 * 1024;
  static const LdsAttr attrs[] = {
      {k_pre<false>, (PackPreFwd::FLOATS + PackPreBwd::FLOATS) * 4}, {k_pre<true>, PRE_LDS_FLOATS * 4}, {k_pre_inp, PackPreInp::FLOATS * 4},
      {k_node_update<8, false>, kUpd}, {k_node_update<8, true>, kUpd}, {k_node_update<8, false, true>, kUpd}, {k_node_update<8, true, true>, kUpd},
      {k_node_update<12, false, false, true>, kUpd3}, {k_node_update<12, true, false, true>, kUpd3},
      {k_node_update<12, false, true, true>, kUpd3}, {k_node_update<12, true, true, true>, kUpd3},
      {k_input_update, PackUpdInp::FLOATS * 4}, {k_score, PackScore::FLOATS * 4},
      {k_gather<false>, k128}, {k_gather<true>, k128}, {k_gather16<false>, k128}, {k_gather16<true>, k128}, {k_gather16<false, true>, k128},
      {k_gather16<false, false, true>, k128}, {k_gather16<true, false, true>, k128},
      {k_livesum, k160}, {k_gather_input_update<true, false>, k160}, {k_gather_input_update<true, true>, k160}, {k_gather<false, true>, k128},
      {k_gather_update_q<16, 0, false>, k160}, {k_gather_update_q<16, 1, false>, k160}, {k_gather_update_q<16, 2, false>, k160},
      {k_gather_update_q<16, 0, false, true>, k160}, {k_gather_update_q<16, 2, false, true>, k160},
      {k_gather_update_q<32, 1, false>, k160}, {k_gather_update_q<32, 1, true>, k160},
      {k_gather_update_q<16, 3, false>, k160}, {k_gather_update_q<32, 3, false>, k160}, {k_gather_update_q<32, 3, true>, k160},
      {k_classify_pre, CLSPRE_LDS_BYTES}, {k_scored_tail, k160 - 256},      // (k_scored_tail also has a few static words)
      {k_top<4>, TOP_LDS_FLOATS * 4}, {k_top<2>, TOP_LDS_FLOATS * 4}, {k_top<1>, TOP_LDS_FLOATS * 4}, {k_babsr, BABSR_LDS_MAX},
  };
  for (const LdsAttr& a : attrs) HIPCHK(hipFuncSetAttribute(a.fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)a.bytes));
  *out = h.release();
  return GNNB_OK;
}

extern "C" int gnnb_destroy(gnnb_t* h) {
  if (!h) return GNNB_OK;
  if (h->work_pool && h->work_pool->owner == getpid()) delete h->work_pool;
  for (auto& ev : h->pending) { (void)hipEventDestroy(ev.a); (void)hipEventDestroy(ev.b); }
  for (auto& ev : h->pool) (void)hipEventDestroy(ev);
  delete h;      // the bound network, the trainer and every buffer go with their owners
  return GNNB_OK;
}

static bool conv_channels_ok(int c) { return c == 3 || c == 8 || c == 16 || c == 32; }

// The handle's helper threads, made on first use: what the machine (or the cgroup's CPU set) offers, a dozen threads with the caller at
// most.  After a fork the parent's threads are not here: its object is left alone and the child gets a pool of its own.
static WorkPool& work_pool(gnnb_t* h) {
  std::lock_guard<std::mutex> lk(h->pool_mutex);
  if (!h->work_pool || h->work_pool->owner != getpid()) {
    const unsigned hc = std::thread::hardware_concurrency();
    cpu_set_t set;
    int avail = (sched_getaffinity(0, sizeof set, &set) == 0) ? CPU_COUNT(&set) : (int)hc;
    if (avail < 1) avail = hc ? (int)hc : 1;
    h->work_pool = new WorkPool(std::max(0, std::min(avail, 12) - 1));
  }
  return *h->work_pool;
}

// gnnb_pack.h check_batch for entry point `who`
static int refuse_batch(const gnnb_t* h, const gnnb_batch* in, int B, const BatchNeeds& need, const char* who) {
  const std::string refusal = check_batch(*h, *in, B, need);
  return refusal.empty() ? GNNB_OK : fail(GNNB_E_INVALID, "%s: %s", who, refusal.c_str());
}

// a network with an inner conv edge that leaves a pixel unread (gnnb_pack.h zero_tap_layer) is refused by the scoring entry points
static int refuse_zero_taps(const gnnb_t* h, const char* who) {
  const int k = h->zero_tap[0], y = h->zero_tap[1], x = h->zero_tap[2];
  if (!k) return GNNB_OK;
  const Edge& e = h->edges[k];
  return fail(GNNB_E_INVALID, "%s: the convolution into ReLU layer %d (%dx%d stride %d pad %d on %dx%d) reads no tap of pixel (%d, %d) of layer %d: "
              "the transposed aggregate is divided by a tap count of 0 there (0/0 in the reference)", who, k, e.kh, e.kw, e.stride, e.pad,
              e.h_in, e.w_in, y, x, k - 1);
}

extern "C" int gnnb_bind_network(gnnb_t* h, const gnnb_layer_desc* L, int n, int c0, int h0, int w0) {
  if (!h || !L || n < 2) return fail(GNNB_E_INVALID, "gnnb_bind_network: bad arguments");
  static_cast<BoundNet&>(*h) = BoundNet();      // the old network goes first; the handle stays unbound unless everything below succeeds
  BoundNet net;
  const std::string refusal = parse_layers(L, n, c0, h0, w0, net);
  if (!refusal.empty()) return fail(GNNB_E_INVALID, "%s", refusal.c_str());
  const int Lr = (int)net.N.size() - 2;
  net.dev.resize(Lr + 1);
  net.kw_w.resize(Lr + 1);
  net.kw_b.resize(Lr + 1);
  fill_kw_geometry(net.kw_net, net);
  for (int k = 1; k <= Lr; ++k) {
    const Edge& e = net.edges[k];
    DevEdge& d = net.dev[k];
    HIPCHK(d.bias.upload(e.b.data(), e.b.size()));
    {                                   // fp64 copies for the fp64 kernels (fp32 -> fp64 is exact); KwNet points at them
      std::vector<double> w64(e.w.begin(), e.w.end()), b64(e.b.begin(), e.b.end());
      HIPCHK(net.kw_w[k].upload(w64.data(), w64.size()));
      HIPCHK(net.kw_b[k].upload(b64.data(), b64.size()));
      net.kw_net.e[k].w = net.kw_w[k].get(); net.kw_net.e[k].bias = net.kw_b[k].get();
    }
    if (k == 1) {                       // k_livesum's job for this edge, done once
      const std::vector<float> s1 = edge1_row_sums(e);
      HIPCHK(net.d_s1.upload(s1.data(), s1.size()));
    }
    if (e.kind == 0) {
      std::vector<float> t(e.w.size());
      pack_conv_fwd(t.data(), e);
      HIPCHK(d.w_fwd.upload(t.data(), t.size()));
      pack_conv_bwd(t.data(), e);
      HIPCHK(d.w_bwd.upload(t.data(), t.size()));
    } else {
      const DenseHost dh = dense_operands(e);
      static_cast<DenseGeom&>(d) = dh.g;
      HIPCHK(d.w_fwd.upload(dh.fwd.data(), dh.fwd.size()));
      HIPCHK(d.w_bwd.upload(dh.bwd.data(), dh.bwd.size()));
    }
  }
  net.top_ok = Lr >= 2 && net.edges[Lr].kind == 1 && net.N[Lr] <= 128 && h->dense_lds && net.dev[Lr].mt_fwd <= 4 && net.dev[Lr].kpad_bwd <= 128;
  // MFMA gather tables for every conv edge, both directions (the input layer's transposed edge is not normalised)
  net.gf.resize(Lr + 1);
  net.gb.resize(Lr + 1);
  if (h->use_gather)
    for (int k = 1; k <= Lr; ++k) {
      if (net.edges[k].kind != 0) continue;
      for (int dir = 0; dir < 2; ++dir) {
        GatherHost gh;
        // the input layer's transposed gather is fused with its feature chain and update (132 MFMAs per tile)
        if (!build_gather(net.edges[k], dir, dir == 1 && k > 1, gh, (dir == 1 && k == 1) ? 132 : 0, /*allow16=*/true)) continue;
        std::vector<int> tt;
        if (!tile_table(gh.g.tm, tt)) return fail(GNNB_E_INVALID, "layer %d: tile table overflow", k);
        // edge 1 forward (dense source rows or the round-0 embedding, never the sparse walk): its tiles in block form where the walk exists
        static_assert(BLK_NCY == kBlocktapRows, "the block-form walk is written for the window rows blocktap_ok asks for");
        if (k == 1 && blocktap_ok(net.edges[k], dir, gh.g)) {
          gh.g.block = BLOCKTAP_FORMS;
          gh.g.ncy = blocktap_rows(net.edges[k]);
          const std::vector<float> img = blocktap_image(net.edges[k], gh.g);
          gh.cmat.insert(gh.cmat.end(), img.begin(), img.end());
        }
        DevGather& d = dir == 0 ? net.gf[k] : net.gb[k];
        d.g = gh.g;
        HIPCHK(d.cmat.upload(gh.cmat.data(), gh.cmat.size()));
        HIPCHK(d.koff.upload(gh.koff.data(), gh.koff.size()));
        HIPCHK(d.ttab.upload(tt.data(), tt.size()));
        d.ok = true;
      }
    }
  // an edge without MFMA gather tables falls back to the VALU gathers, which are compiled for a few channel counts only
  for (int k = 1; k <= Lr; ++k) {
    const Edge& e = net.edges[k];
    if (e.kind != 0) continue;
    if ((!net.gf[k].ok && !conv_channels_ok(e.c_out)) || (!net.gb[k].ok && !conv_channels_ok(e.c_in)))
      return fail(GNNB_E_INVALID, "conv edge %d (%d -> %d channels): no MFMA gather tables and the fallback kernels only cover channel counts "
                  "{3, 8, 16, 32}", k, e.c_in, e.c_out);
  }
  net.zero_tap[0] = zero_tap_layer(net, &net.zero_tap[1], &net.zero_tap[2]);
  net.bound = true;
  static_cast<BoundNet&>(*h) = std::move(net);
  for (int k = 0; k < MAXL + 2; ++k) h->last_proj[k] = -1;
  return GNNB_OK;
}

// tile map of the input layer's update: the tiles of the transposed gather of edge 1 when it exists, else flat
static TileMap flat_map(int N) { TileMap t; t.mode = 0; t.N = N; return t; }
static TileMap bwd_map(const gnnb_t* h, int k) {
  const int L = (int)h->N.size() - 2;
  return (k + 1 <= L && h->gb[k + 1].ok) ? h->gb[k + 1].g.tm : flat_map(h->N[k]);
}
static long map_tiles(const TileMap& t, int B) { return t.mode ? (long)B * t.TPS : ((long)B * t.N + 31) / 32; }
static int ilog2(int v) { int l = 0; while ((1 << l) < v) ++l; return l; }
static int pairs_per_sample(const TileMap& t) { return t.NCG * ((t.NBY + 1) / 2) * t.NBX; }      // row pairs of the block-form tiles (fusedq_gather_pairs)
static DTileMap to_dtm(const TileMap& t) {
  const int pps = t.mode ? pairs_per_sample(t) : 0;
  return DTileMap{t.mode, t.N, t.C, t.H, t.W, t.CT, t.PY, t.PX, t.ay, t.ax, t.NBY, t.NBX, t.NCG, t.TPS, ilog2(t.PY), ilog2(t.PX),
                  t.TPS > 1 ? (unsigned)((1ull << 32) / (unsigned)t.TPS) + 1u : 0u,      // tile_sample (gnnb_dev.h); TPS <= 1 is handled there
                  pps, pps > 1 ? (unsigned)((1ull << 32) / (unsigned)pps) + 1u : 0u};     // pair_sample
}
// rows of 64 floats of an edge's tap images in LDS: the tap matrix, and behind it the block-form image where the edge has one
static int cm_rows(const GatherGeom& g) { return g.tm.NCG * (g.K2 + (g.block ? g.ncy : 0)); }
static DGather to_dg(const DevGather& d, const float* zero) {
  const GatherGeom& g = d.g;
  return DGather{d.cmat.get(), reinterpret_cast<const int2*>(d.koff.get()), d.ttab.get(), zero, g.K2, cm_rows(g), g.Hs, g.Ws, g.Ns, g.ystep, g.ybase,
                 g.xstep, g.xbase, g.WY, g.WX, g.normalise, g.kh, g.kw, g.stride, g.pad, g.lanes, g.block, g.tm.NCG * g.K2 * 64};
}
static size_t gather_lds_bytes(const DevGather& d, size_t pack_floats) {
  return (pack_floats + (size_t)cm_rows(d.g) * 64) * 4 + (size_t)gather_slots(d.g.K2, d.g.lanes) * 12 + (size_t)((d.g.tm.TPS + 3) & ~3) * 4;
}

// per-wave live-slot tables of the sparse gathers (behind the shared tables, 8-byte aligned)
static size_t sparse_tab_bytes(const DevGather& d) {
  return 8 + (size_t)WAVES_MLP * ((d.g.lanes == 16 ? 4 : 2) * d.g.K2 + 32) * 8;
}

#if defined(FUSED_TIMING) && FUSED_TIMING == 6
// dev: start / end (100 MHz chip-wide clock) of every wave of the instrumented k_gather_update_q launch: 2 x 16 x gridDim words
extern "C" int gnnb_debug_wall(unsigned long long* out, int nwords) {
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_qt_wall), (size_t)nwords * 8) == hipSuccess ? 0 : -1;
}
#endif
#ifdef FUSED_TIMING
// dev: cycle sums of k_gather_update's phases over every wave since the last reset (index 15: number of waves)
extern "C" int gnnb_debug_read(unsigned long long* out, int reset) {
  unsigned long long z[16] = {0};
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_fused_t), sizeof z) != hipSuccess) return -1;
  if (reset && hipMemcpyToSymbol(HIP_SYMBOL(g_fused_t), z, sizeof z) != hipSuccess) return -1;
  return 0;
}
#endif

extern "C" int gnnb_graph_info(const gnnb_t* h, int* n_graph, int* sizes, int* n_relu_total) {
  if (!h || !h->bound) return fail(GNNB_E_STATE, "gnnb_graph_info: no network bound");
  if (n_graph) *n_graph = (int)h->N.size();
  if (sizes)
    for (size_t k = 0; k < h->N.size(); ++k) sizes[k] = h->N[k];
  if (n_relu_total) *n_relu_total = h->R;
  return GNNB_OK;
}

// k_gather_update_q over conv edge `d`: dynamic LDS bytes (weights, row queue, gather tables, per-gather-wave slot tables), and
// whether the edge can take it at all (a sparse walk behind a ReLU layer, 16-node tiles without POST, everything in 160 KB)
static size_t fusedq_lds_bytes(const DevGather& d, bool sparse, bool post, int qtiles) {
  const size_t tables = (size_t)cm_rows(d.g) * 64 * 4 + (size_t)gather_slots(d.g.K2, d.g.lanes) * 8 + (size_t)((d.g.tm.TPS + 3) & ~3) * 4 +
                        (size_t)((gather_slots(d.g.K2, d.g.lanes) + 3) & ~3) * 4;
  return (size_t)(PackUpdL3::FLOATS + (post ? 6144 : 0) + fusedq_queue_floats(qtiles)) * 4 + tables +
         (sparse ? (size_t)QG_WAVES * ((d.g.lanes == 16 ? 4 : 2) * d.g.K2 + 32) * 8 : 0);
}
// ring slots that fit (0: the kernel does not fit at all)
static int fusedq_qtiles(const DevGather& d, bool sparse, bool post) {
  for (int q = QTILES; q >= 2; --q)
    if (fusedq_lds_bytes(d, sparse, post, q) <= 160 * 1024) return q;
  return 0;
}
static bool fusedq_ok(const gnnb_t* h, const DevGather& d, int src_layer, bool embed_src, bool post) {
  if (h->fuse == 0 || !h->bf3 || !d.ok) return false;
  const bool sparse = !embed_src && src_layer >= 1;
  if (src_layer >= 1 && !sparse) return false;
  if (d.g.lanes == 32 && !sparse) return false;
  if (d.g.lanes == 16 && post) return false;
  return fusedq_qtiles(d, sparse, post) > 0;
}

// the scored gather (k_gather_scored, k_scored_tail) keeps a node's source window in registers: C_out x ceil(kh/s) x ceil(kw/s) slots
static int gs_slots(const Edge& e) { return e.c_out * ((e.kh + e.stride - 1) / e.stride) * ((e.kw + e.stride - 1) / e.stride); }
static bool gs_window_ok(const Edge& e) { return gs_slots(e) <= GS_SLOT_LIMIT; }

#define TOP_SPLIT_MAXB 128      // k_top only splits a sample over workgroups while B x S workgroups fit the chip: B <= n_cu / 2

// What gnnb_forward decides before its first launch, from the handle, the batch size and the half-pass limit alone.
// gnnb_describe reads its decisions from the same plan (with no limit).
struct Plan {
  int limit;                // half-passes to run: 2 T, or fewer under an inspection limit
  bool debug_full;          // a half-pass limit is set: nothing is restricted or skipped as dead
  bool top_fused;           // the top of the network in k_top
  bool top_upd;             // ... which also runs the backward node update of layer L-1
  bool top_s_fwd, top_s_bwd;  // ... and produces the bias sums of edge L forward / transposed itself
  bool s1_table;            // bias sums of edge 1 forward: the bind-time table
  bool embed_in_gather;     // round 0's input embedding computed inside the first forward gather (no k_embed)
  bool cls_pre;             // k_classify and k_pre in one launch (k_classify_pre)
  bool need_inp;            // k_pre_inp: the input layer's feature chain for the non-fused input update
  bool tail;                // the final round's restricted update of layer 1 and the score head in one launch (k_scored_tail)
  int S;                    // workgroups k_top spreads one sample over
};
static Plan make_plan(const gnnb_t* h, int B, int halfpass_limit) {
  const int L = (int)h->N.size() - 2;
  Plan p;
  p.limit = halfpass_limit > 0 ? std::min(halfpass_limit, 2 * h->T) : 2 * h->T;
  p.debug_full = halfpass_limit > 0;
  // The one-workgroup-per-sample kernels (k_top, k_dense_*_lds) run at every batch size, although a small batch leaves CUs idle
  // (per-tile kernels vs these: B=2 0.40 vs 0.49 ms, B=128 0.96 vs 0.88 ms): the two paths round differently, and with one path
  // for every batch size a sample's scores do not depend on what it is batched or sharded with.
  p.top_fused = h->use_top && h->bf3 && h->top_ok && !p.debug_full;      // (k_top only exists on the bf16 x 3 rate)
  // k_top's Linear edges walk live rows only (when their lists fit, top_sample `compact` / `keep`), so they produce the bias sums
  // of edge L in both directions themselves and k_livesum skips those jobs
  const int topK = L >= 1 && h->edges[L].kind == 1 ? h->edges[L].n_in : 0;
  p.top_s_fwd = p.top_fused && TOP_LIST_OK(topK);
  p.top_s_bwd = p.top_fused && TOP_LIST_KEEP_OK(topK) && p.limit >= 2;
  // k_top also runs the backward node update of layer L-1 on its transposed edge's row tiles (the aggregate never reaches memory):
  // needs the kept live-row list (B2 then walks live rows only) and a layer L-1 that is not layer 1 (whose update has the
  // restricted / input-mapping forms)
  p.top_upd = p.top_fused && h->top_fuse_upd && L >= 3 && TOP_LIST_KEEP_OK(topK);
  p.s1_table = L >= 2 && h->d_s1.get() != nullptr;
  p.embed_in_gather = h->embed_fuse && !p.debug_full && h->gf[1].ok;
  p.cls_pre = h->bf3 && B <= h->clspre_max_b;      // default: a single subproblem
  p.need_inp = p.limit >= 2 && (h->T > 1 || p.debug_full) && !h->gb[1].ok;    // the fused input kernel computes Q itself
  // the final round's scored update of layer 1 as k_scored_tail: on the k_top path only, with layer 1 below the layer whose aggregate
  // k_top leaves in `nb` (L >= 3), over a conv edge 2 with MFMA gather tables and a window the scored gather holds
  p.tail = p.top_fused && L >= 3 && B <= h->tail_max_b && h->edges[2].kind == 0 && h->gb[2].ok && gs_window_ok(h->edges[2]) && h->N[2] < 65536;
  // A sample's top spread over S = 2 / 4 workgroups (by output tile of both Linear edges) while all B x S of them are resident
  // at one per CU (they wait for each other); the top_split option caps S.  The results do not depend on S.
  // S = 4 while B <= n_cu / 4 (base B = 1: 52 -> 38 us per launch), S = 2 while B <= n_cu / 2.  (Before k_top also ran the update of
  // layer L-1, S = 2 was a draw -- the two hand-offs cost what the shorter edges saved; with the update's tiles split over both
  // workgroups too it wins: deep B = 128 67 -> 59 us, wide B = 128 99 -> 79 us per launch.)  topflag / xbuf are sized for
  // TOP_SPLIT_MAXB samples.
  p.S = 1;
  if (h->top_split_max >= 4 && (long)B * 4 <= h->n_cu && B <= TOP_SPLIT_MAXB) p.S = 4;
  else if (h->top_split_max >= 2 && (long)B * 2 <= h->n_cu && B <= TOP_SPLIT_MAXB) p.S = 2;
  return p;
}

// JSON description of the launch plan of one forward (per B=1): which kernel updates which layer, tile shapes and
// MFMA counts.  bench.py derives the algorithmic flops per kernel class from it; DESIGN.md quotes it.
extern "C" int gnnb_describe(const gnnb_t* h, char* buf, size_t cap) {
  if (!h || !h->bound || !buf || cap < 64) return fail(GNNB_E_INVALID, "gnnb_describe: bad arguments");
  const int L = (int)h->N.size() - 2;
  const Plan p = make_plan(h, 1, 0);
  std::string o = "{\"T\": " + std::to_string(h->T) + ", \"bf3\": " + std::to_string(h->bf3 ? 1 : 0) + ", \"embed_fused\": " + std::to_string(p.embed_in_gather ? 1 : 0) + ", \"sizes\": [";
  for (size_t k = 0; k < h->N.size(); ++k) o += (k ? ", " : "") + std::to_string(h->N[k]);
  o += "], \"updates\": [";
  auto nnz = [&](int e) -> long {     // edges of the layer graph between layer e-1 and e (no-padding upper bound)
    if (e > L) return h->N[L];
    const Edge& ed = h->edges[e];
    return ed.kind == 0 ? (long)ed.c_out * ed.h_out * ed.w_out * ed.c_in * ed.kh * ed.kw : (long)ed.n_in * ed.n_out;
  };
  auto item = [&](const char* what, int k, const DevGather* d, const char* fallback, int n_src) {
    char t[640];
    const long ez = nnz(what[0] == 'f' ? k : k + 1);
    if (d && d->ok) {
      const GatherGeom& g = d->g;
      snprintf(t, sizeof t,
               "{\"update\": \"%s\", \"layer\": %d, \"kernel\": \"%s\", \"nodes\": %d, \"tiles_per_sample\": %d, \"tile_nodes\": %d, "
               "\"tile\": [%d, %d, %d], \"align\": [%d, %d], \"window\": [%d, %d], \"gather_ksteps\": %d, \"n_src\": %d, \"edge_nnz\": %ld}",
               what, k, k == 0 ? "k_gather_input_update" : (fusedq_ok(h, *d, what[0] == 'f' ? k - 1 : k + 1, false, false) ? "k_gather_update" : "k_gather+k_node_update"),
               h->N[k], g.tm.TPS, g.lanes, g.tm.CT, g.tm.PY, g.tm.PX,
               g.tm.ay, g.tm.ax, g.WY, g.WX, g.K2, n_src, ez);
    } else {
      snprintf(t, sizeof t, "{\"update\": \"%s\", \"layer\": %d, \"kernel\": \"%s\", \"nodes\": %d, \"n_src\": %d, \"edge_nnz\": %ld}",
               what, k, fallback, h->N[k], n_src, ez);
    }
    o += t;
  };
  const bool top = p.top_fused;     // k_top covers the edge into layer L, both updates of layer L and the edge back
  bool first = true;
  for (int k = 1; k <= L; ++k) {
    if (!first) o += ", ";
    first = false;
    if (top && k == L) item("fwd", k, nullptr, "k_top+k_top", h->N[k - 1]);
    else item("fwd", k, &h->gf[k], h->edges[k].kind == 0 ? "k_conv_fwd+k_node_update" : "k_dense_agg+k_node_update", h->N[k - 1]);
  }
  for (int k = L; k >= 1; --k) {
    o += ", ";
    if (k == L) item("bwd", k, nullptr, top ? "k_top+k_top" : "k_prop+k_node_update", 1);
    else if (top && k == L - 1)      // (the update of layer L-1 rides k_top's transposed edge when its live-row list is kept: Plan::top_upd)
      item("bwd", k, nullptr, p.top_upd ? "k_top+k_top" : "k_top+k_node_update", h->N[k + 1]);
    else item("bwd", k, &h->gb[k + 1], h->edges[k + 1].kind == 0 ? "k_convT_bwd+k_node_update" : "k_dense_agg+k_node_update", h->N[k + 1]);
  }
  o += ", ";
  item("input", 0, &h->gb[1], h->edges[1].kind == 0 ? "k_convT_bwd+k_input_update" : "k_dense_agg+k_input_update", h->N[1]);
  o += "]}";
  if (o.size() + 1 > cap) return fail(GNNB_E_NOMEM, "gnnb_describe: buffer too small (%zu needed)", o.size() + 1);
  memcpy(buf, o.c_str(), o.size() + 1);
  return GNNB_OK;
}

// ---- workspace layout (float offsets, every region 256-B aligned) ----
struct WsLayout {                // plain arrays: gnnb_forward computes it on its stack (no allocation in the call)
  size_t mu[MAXL + 2], Pf[MAXL + 2], Pb[MAXL + 2], live[MAXL + 2], amb[MAXL + 2], score[MAXL + 2];
  size_t lf[MAXL + 2];          // live flags (B, N_k) as floats
  size_t lbits[MAXL + 2];       // the same flags one bit per node (k_classify's ballots), read as 32-bit words by the sparse gathers (BitsLive); inside Q
  bool bits = false;            // the bitmaps have a place (else k_classify writes none and every sparse table build reads the bounds)
  size_t sf[MAXL + 2], sb[MAXL + 2];   // k_livesum outputs: sf[k] (B, N_k) over edge k, sb[k] (B, N_k) over edge k+1 transposed
  size_t F1 = 0;                // rows of layer 1 after the producer-side map of the input update (PackPostInp)
  size_t cnt = 0, best = 0, nb = 0, Q = 0, total = 0;     // best: B 64-bit decision keys + the finished-workgroup counter of k_score
  size_t topflag = 0, topx = 0;                           // k_top's workgroup split: arrival counters, (B, 8, 64) exchange buffer
};
static size_t align64(size_t nfloats) { return (nfloats + 63) & ~(size_t)63; }
static WsLayout ws_layout(const gnnb_t* h, int B) {
  WsLayout w;
  for (int k = 0; k < MAXL + 2; ++k) w.mu[k] = w.Pf[k] = w.Pb[k] = w.live[k] = w.amb[k] = w.score[k] = w.lf[k] = w.lbits[k] = w.sf[k] = w.sb[k] = 0;
  const int K = (int)h->N.size() - 1;
  size_t off = 0;
  w.cnt = off; off += 64;                      // (unused: the list counters live in the handle's control blocks)
  w.best = off; off += align64((size_t)2 * B + 2);
  w.topflag = off; off += align64(TOP_SPLIT_MAXB);
  w.topx = off; off += align64((size_t)std::min(B, TOP_SPLIT_MAXB) * 512);
  for (int k = 0; k <= K; ++k) { w.mu[k] = off; off += align64((size_t)B * h->N[k] * 64); }
  size_t maxn = 0;
  for (int k = 0; k < K; ++k) maxn = std::max(maxn, (size_t)h->N[k]);
  w.nb = off; off += align64((size_t)B * maxn * 64);
  for (int k = 1; k < K; ++k) { w.Pf[k] = off; off += align64((size_t)B * h->N[k] * 64); }
  for (int k = 1; k < K; ++k) { w.Pb[k] = off; off += align64((size_t)B * h->N[k] * 64); }
  for (int k = 1; k < K; ++k) {
    w.live[k] = off; off += align64((size_t)B * h->N[k]);
    w.amb[k] = off; off += align64((size_t)B * h->N[k]);
    w.score[k] = off; off += align64((size_t)B * h->N[k]);
  }
  for (int k = 1; k < K; ++k) { w.lf[k] = off; off += align64((size_t)B * h->N[k]); }
  for (int k = 1; k < K; ++k) { w.sf[k] = off; off += align64((size_t)B * h->N[k]); }
  for (int k = 0; k < K - 1; ++k) { w.sb[k] = off; off += align64((size_t)B * h->N[k]); }
  w.F1 = off; off += align64((size_t)B * h->N[1] * 64);
  w.Q = off; off += (size_t)map_tiles(bwd_map(h, 0), B) * 2048;
  w.total = off;
  // The live bitmaps take the front of Q, which only the unfused input update writes and reads (k_pre_inp, k_input_update: no transposed
  // gather tables on edge 1), so the workspace keeps its size.  Per ReLU layer: ceil(B N_k / 64) 64-bit words, then LIVEBITS_PAD 32-bit
  // words nobody writes -- a gather wave reads the 64 words from its sample's first one on without a guard (the words behind the sample's
  // last node are never selected).
  if (K >= 2 && h->gb[1].ok) {
    size_t o = w.Q;
    for (int k = 1; k < K; ++k) { w.lbits[k] = o; o += align64(2 * (((size_t)B * h->N[k] + 63) / 64) + LIVEBITS_PAD); }
    w.bits = o <= w.total;
  }
  return w;
}

extern "C" size_t gnnb_workspace_bytes(const gnnb_t* h, int B) {
  if (!h || !h->bound || B < 1) return 0;
  return ws_layout(h, B).total * sizeof(float);
}

extern "C" int gnnb_mu_location(const gnnb_t* h, int B, int k, size_t* offset_bytes, size_t* n_floats) {
  if (!h || !h->bound) return fail(GNNB_E_STATE, "gnnb_mu_location: no network bound");
  if (k < 0 || k >= (int)h->N.size() || B < 1) return fail(GNNB_E_INVALID, "gnnb_mu_location: bad layer/batch");
  WsLayout w = ws_layout(h, B);
  if (offset_bytes) *offset_bytes = w.mu[k] * sizeof(float);
  if (n_floats) *n_floats = (size_t)B * h->N[k] * 64;
  return GNNB_OK;
}

// Inspection: the rows of mu[k] written by the last forward are E with mu = W.E + b for the Linear `*linear_id`
// (index into the checkpoint's 26 Linear layers in state-dict order), or final embeddings when *linear_id = -1.
extern "C" int gnnb_mu_projection(const gnnb_t* h, int k, int* linear_id) {
  if (!h || !linear_id) return fail(GNNB_E_INVALID, "gnnb_mu_projection: null argument");
  if (k < 0 || k >= (int)h->N.size()) return fail(GNNB_E_INVALID, "gnnb_mu_projection: bad layer");
  *linear_id = k < MAXL + 2 ? h->last_proj[k] : -1;
  return GNNB_OK;
}

extern "C" int gnnb_set_halfpass_limit(gnnb_t* h, int n) {
  if (!h) return fail(GNNB_E_INVALID, "null handle");
  h->halfpass_limit = n;
  return GNNB_OK;
}

// Inspection: occupy `n_workgroups` CUs (one workgroup each when lds_bytes > 80 KiB) for `ms` milliseconds (<= 500) on `stream` with a kernel that
// only spins on the clock -- the stand-in for "something else holds CUs" (an RCCL kernel, a second batch) in tests/test_gpu_dist_safety.py.
extern "C" int gnnb_debug_occupy(int n_workgroups, int threads, size_t lds_bytes, double ms, void* stream) {
  if (n_workgroups < 1 || n_workgroups > 4096 || threads < 64 || threads > 1024 || lds_bytes > 160 * 1024 || !(ms > 0.0) || ms > 500.0)
    return fail(GNNB_E_INVALID, "gnnb_debug_occupy: bad arguments");
  static bool attr = false;
  if (!attr) { HIPCHK(hipFuncSetAttribute((const void*)k_occupy, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024)); attr = true; }
  hipLaunchKernelGGL(k_occupy, dim3((unsigned)n_workgroups), dim3((unsigned)threads), lds_bytes, (hipStream_t)stream, (unsigned long long)(ms * 1e5));
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(GNNB_E_HIP, "launch of k_occupy failed: %s", hipGetErrorString(e));
  return GNNB_OK;
}

// ---- profiling ----
extern "C" int gnnb_profile_enable(gnnb_t* h, int on) {
  if (!h) return fail(GNNB_E_INVALID, "null handle");
  h->prof = on != 0;
  return GNNB_OK;
}
extern "C" int gnnb_profile_classes(void) { return PC_COUNT; }
extern "C" const char* gnnb_profile_class_name(int cls) { return (cls >= 0 && cls < PC_COUNT) ? kProfNames[cls] : ""; }
extern "C" int gnnb_profile_read(gnnb_t* h, double* total_ms, int64_t* launches, int n, int reset) {
  if (!h) return fail(GNNB_E_INVALID, "null handle");
  if (!h->pending.empty()) {
    for (auto& ev : h->pending) {
      HIPCHK(hipEventSynchronize(ev.b));        // launches may sit on several streams (batch pipelining)
      float ms = 0.f;
      HIPCHK(hipEventElapsedTime(&ms, ev.a, ev.b));
      h->prof_ms[ev.cls] += ms;
      h->prof_n[ev.cls] += 1;
      if (h->trace.size() < 65536) h->trace.push_back({ev.cls, ms});
      h->pool.push_back(ev.a);
      h->pool.push_back(ev.b);
    }
    h->pending.clear();
  }
  for (int i = 0; i < n && i < PC_COUNT; ++i) {
    if (total_ms) total_ms[i] = h->prof_ms[i];
    if (launches) launches[i] = h->prof_n[i];
  }
  if (reset)
    for (int i = 0; i < PC_COUNT; ++i) { h->prof_ms[i] = 0; h->prof_n[i] = 0; }
  return GNNB_OK;
}
// The launches gnnb_profile_read has resolved since the last call of this function, in launch order: class and duration of each
// (bench.py prices single launches of a class with it).  Returns their number (at most cap are copied); the list is cleared.
extern "C" int gnnb_profile_trace(gnnb_t* h, int* cls, double* ms, int cap) {
  if (!h) { fail(GNNB_E_INVALID, "null handle"); return -1; }
  const int n = (int)h->trace.size();
  for (int i = 0; i < n && i < cap; ++i) {
    if (cls) cls[i] = h->trace[i].cls;
    if (ms) ms[i] = h->trace[i].ms;
  }
  h->trace.clear();
  return n;
}

struct Launcher {
  gnnb_t* h;
  hipStream_t st;
  int rc = 0;
  hipEvent_t get_event() {
    if (!h->pool.empty()) { hipEvent_t e = h->pool.back(); h->pool.pop_back(); return e; }
    hipEvent_t e = nullptr;
    if (hipEventCreate(&e) != hipSuccess) rc = fail(GNNB_E_HIP, "hipEventCreate failed");
    return e;
  }
  template <class F>
  void run(int cls, F&& f) {
    if (rc) return;
    if (h->prof) {
      gnnb_handle::Ev ev{cls, get_event(), get_event()};
      if (rc) return;
      (void)hipEventRecord(ev.a, st);
      f();
      (void)hipEventRecord(ev.b, st);
      h->pending.push_back(ev);
      h->prof_stream = st;
    } else {
      f();
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) rc = fail(GNNB_E_HIP, "launch of %s failed: %s", kProfNames[cls], hipGetErrorString(e));
  }
};

static int mlp_grid(const gnnb_t* h, long ntiles) {
  long g = (ntiles + WAVES_MLP - 1) / WAVES_MLP;
  if (g > h->n_cu) g = h->n_cu;
  return (int)(g < 1 ? 1 : g);
}

// The aggregates of edges without MFMA gather tables.  VALU conv kernels, compiled for the channel counts bind admits: by output
// channels forward, by input channels transposed (anything else than 3, 8, 16 takes the 32-channel form).  The per-tile Linear
// kernel: [0] splits K (K >= 512), [1] does not.  (The order of the three tables is the order the kernels have in the code object.)
static void (*const kConvFwd[4])(ConvArgs) = {k_conv_fwd<3>, k_conv_fwd<8>, k_conv_fwd<16>, k_conv_fwd<32>};
static void (*const kDenseAgg[2])(DenseArgs) = {k_dense_agg<true>, k_dense_agg<false>};
static void (*const kConvT[4])(ConvArgs) = {k_convT_bwd<3>, k_convT_bwd<8>, k_convT_bwd<16>, k_convT_bwd<32>};
static int conv_channel_form(int c) { return c == 3 ? 0 : c == 8 ? 1 : c == 16 ? 2 : 3; }

// The launches of one gnnb_forward call: the call's arguments, its workspace and its plan, and one method per launch (or choice of
// launch) of a forward.  It lives on gnnb_forward's stack; proj[] is the deferred projection of the rows of mu[k] after the kernels
// enqueued so far (gnnb_pack.h).
struct Forward {
  gnnb_t* h;
  const gnnb_batch* in;
  int B, K, L;
  const Plan& p;
  const WsLayout& w;
  float* ws;
  float* scores;
  int32_t* decisions;
  int32_t* status;
  hipStream_t st;
  int* cnt;                         // the list counters (the control block of this workspace, gnnb_handle::d_ctl)
  Launcher lz;
  float* nb;
  // The rows of layer 1 the input-layer update aggregates went through its 64x64 map on the producer side (PackPostInp).
  // Outside inspection runs nothing else reads the plain rows of that half-pass, so the mapped rows simply take their place
  // in mu[1] (whose dead rows k_classify already zeroed); inspection runs keep both, the mapped ones in F1.
  float* rows1_for_input;
  int roff[MAXL + 2] = {0};         // offset of layer k inside the flat ReLU index
  int proj[MAXL + 2];
  int top_launches = 0;

  Forward(gnnb_t* h_, const gnnb_batch* in_, int B_, const Plan& p_, const WsLayout& w_, void* workspace, float* scores_, int32_t* decisions_,
          int32_t* status_, hipStream_t st_, int* cnt_)
      : h(h_), in(in_), B(B_), K((int)h_->N.size() - 1), L(K - 1), p(p_), w(w_), ws((float*)workspace), scores(scores_), decisions(decisions_),
        status(status_), st(st_), cnt(cnt_), lz{h_, st_}, nb(ws + w_.nb), rows1_for_input(p_.debug_full ? ws + w_.F1 : ws + w_.mu[1]) {
    for (int k = 2; k <= L + 1; ++k) roff[k] = roff[k - 1] + h->N[k - 1];
    for (int k = 0; k < MAXL + 2; ++k) proj[k] = -1;
  }
  float* mu(int k) const { return ws + w.mu[k]; }
  int* ilist(size_t off) const { return reinterpret_cast<int*>(ws + off); }
  unsigned long long* best() const { return reinterpret_cast<unsigned long long*>(ws + w.best); }
  int* done_ctr() const { return reinterpret_cast<int*>(ws + w.best + 2 * (size_t)B); }

  // The rows of dead nodes are zero by definition (mu = (.) * live).  Every default consumer of a layer's rows walks only the
  // live ones (sparse gathers, the compacted Linear edges of k_top, the score head), so nothing needs them in memory; they
  // are written (k_classify) only for a layer with a consumer that reads every row: VALU / non-sparse gathers, the
  // per-sample / per-tile dense kernels, k_prop, inspection runs.
  bool reads_live_rows_only(int e, bool transposed) const {      // edge e between layers e-1 and e; transposed: reads layer e
    if (e == L && p.top_fused) return transposed || TOP_LIST_OK(h->edges[L].n_in);
    return (transposed ? h->gb[e] : h->gf[e]).ok;
  }
  bool zero_dead_rows(int k) const {
    if (p.debug_full) return true;
    if (k == L) return !p.top_fused;                                // k_top writes every row of layer L itself
    return !(reads_live_rows_only(k + 1, false) && reads_live_rows_only(k, true));
  }

  // ---- once per forward: classification lists, bias sums, input embedding, embedding-independent feature chains ----
  PreAllArgs pre_args() const {
    PreAllArgs a{};
    a.pack_f = h->d_pack[PK_PRE_FWD]; a.pack_b = h->d_pack[PK_PRE_BWD];
    a.L = L; a.do_bwd = p.limit >= 2 ? 1 : 0; a.cnt = cnt + 4;
    for (int k = 1; k <= L; ++k) {
      const int i = k - 1;
      const ReluRows r = relu_rows(*h, *in, B, k);
      a.lb[i] = r.lb; a.ub[i] = r.ub; a.dual[i] = r.dual; a.z_pre[i] = r.z_pre; a.z_post[i] = r.z_post; a.bias[i] = h->dev[k].bias.get();
      a.Pf[i] = ws + w.Pf[k]; a.Pb[i] = ws + w.Pb[k]; a.list[i] = ilist(w.amb[k]);
      a.N[i] = h->N[k]; a.hw[i] = h->hw[k];
    }
    return a;
  }
  void classify() {
    ClassifyArgs a{};
    a.L = L; a.mask = in->mask; a.scores = scores; a.cnt = cnt + 4; a.R = h->R;
    a.status = status; a.best = best(); a.done = done_ctr(); a.B = B;
    a.topflag = reinterpret_cast<int*>(ws + w.topflag); a.nflag = std::min(B, TOP_SPLIT_MAXB);
    a.mu2 = p.debug_full ? ws + w.F1 : nullptr;      // inspection runs keep the plain rows in mu[1] and the mapped ones in F1
    int blk = 0;
    for (int k = 1; k <= L; ++k) {
      const int i = k - 1;
      a.lb[i] = in->lb[k]; a.ub[i] = in->ub[k]; a.mu[i] = mu(k); a.zero[i] = zero_dead_rows(k) ? 1 : 0;
      a.live[i] = ilist(w.live[k]); a.amb[i] = ilist(w.amb[k]); a.score[i] = ilist(w.score[k]);
      a.livef[i] = ws + w.lf[k];
      a.lbits[i] = w.bits ? reinterpret_cast<unsigned long long*>(ws + w.lbits[k]) : nullptr;
      a.G[i] = (long)B * h->N[k]; a.N[i] = h->N[k]; a.off[i] = roff[k];
      a.blk0[i] = blk;
      blk += (int)((a.G[i] + CLS_BLOCK - 1) / CLS_BLOCK);
    }
    a.blk0[L] = blk;
    if (p.cls_pre) {
      const PreAllArgs pre = pre_args();
      lz.run(PC_CLASSIFY, [&] { hipLaunchKernelGGL(k_classify_pre, dim3((unsigned)blk), dim3(CLS_THREADS), CLSPRE_LDS_BYTES, st, a, pre); });
    } else {
      lz.run(PC_CLASSIFY, [&] { hipLaunchKernelGGL(k_classify, dim3((unsigned)blk), dim3(CLS_THREADS), 0, st, a); });
    }
  }
  void livesum() {   // bias-sum scalars of every edge and direction (the rows carry deferred projections)
    LiveSumArgs a{};
    a.B = B;
    int q = 0, maxw = 0;
    auto push = [&](int kind, const Edge& e, const float* wt, int ld, const float* lf, float* out, int Ndst, int Nsrc, int normalise) {
      LiveSumJob& j = a.job[q++];
      j.kind = kind; j.w = wt; j.lf = lf; j.out = out; j.Ndst = Ndst; j.Nsrc = Nsrc; j.ld = ld; j.normalise = normalise;
      j.c_in = e.c_in; j.h_in = e.h_in; j.w_in = e.w_in; j.c_out = e.c_out; j.h_out = e.h_out; j.w_out = e.w_out;
      j.kh = e.kh; j.kw = e.kw; j.stride = e.stride; j.pad = e.pad;
      const long nw = (long)e.c_in * e.c_out * e.kh * e.kw;
      j.wlds = (e.kind == 0 && nw <= LIVESUM_MAXW) ? (int)nw : 0;
      maxw = std::max(maxw, j.wlds);
    };
    // edges whose aggregate comes from a sparse gather get their bias sums from that gather (GArgs.sout / GIArgs.s_from_gather)
    for (int k = 1; k <= L; ++k) {            // forward edge k: source layer k-1 (the input layer is all live)
      const Edge& e = h->edges[k];
      if (k == 1 && p.s1_table) continue;
      if (k >= 2 && h->gf[k].ok) continue;
      if (k == L && p.top_s_fwd) continue;
      push(e.kind == 0 ? 0 : 1, e, e.kind == 0 ? h->dev[k].w_fwd.get() : h->dev[k].w_bwd.get(), h->dev[k].ld_bwd, k > 1 ? ws + w.lf[k - 1] : nullptr,
           ws + w.sf[k], h->N[k], h->N[k - 1], 0);
    }
    if (p.limit >= 2)
      for (int k = 0; k < L; ++k) {           // edge k+1 transposed: source layer k+1
        const Edge& e = h->edges[k + 1];
        if (h->gb[k + 1].ok) continue;
        if (k == L - 1 && p.top_s_bwd) continue;
        push(e.kind == 0 ? 2 : 3, e, h->dev[k + 1].w_bwd.get(), h->dev[k + 1].ld_bwd, ws + w.lf[k + 1], ws + w.sb[k], h->N[k], h->N[k + 1],
             k >= 1 ? 1 : 0);
      }
    a.njobs = q;
    if (q == 0) return;                 // every edge's bias sums come from its gather, k_top or the bind-time table
    int maxn = 0;
    for (int k = 0; k <= L; ++k) maxn = std::max(maxn, h->N[k]);
    a.lv_floats = (maxn + 3) & ~3;
    if ((size_t)(a.lv_floats + maxw) * 4 > 160 * 1024) {      // very wide layers: leave the weights in global memory
      for (int i = 0; i < q; ++i) a.job[i].wlds = 0;
      maxw = 0;
    }
    // (running this and k_pre on a side stream under k_embed / the first aggregation was measured: 1.72 ms vs 1.59 ms in-line)
    lz.run(PC_LIVESUM, [&] { hipLaunchKernelGGL(k_livesum, dim3((unsigned)B, (unsigned)q), dim3(256), (size_t)(a.lv_floats + maxw) * sizeof(float), st, a); });
  }
  void input_embedding() {
    const long G = (long)B * h->N[0];
    EmbedArgs a{h->d_pack[PK_EMBED] + PackEmbed::W, h->d_pack[PK_EMBED] + PackEmbed::B, in->lb[0], in->x_lp, in->ub[0], mu(0), G};
    long grid = (G + 16 * EMBED_UNROLL - 1) / (16 * EMBED_UNROLL);
    if (grid > (long)h->n_cu * 16) grid = (long)h->n_cu * 16;
    // with the MFMA gather on the first edge, round 0 computes the embedding inside that gather (k_gather<true>): nothing
    // else reads mu[0] before the input-layer update overwrites it.  Inspection runs keep the rows.
    if (!p.embed_in_gather) lz.run(PC_EMBED, [&] { hipLaunchKernelGGL(k_embed, dim3((unsigned)grid), dim3(256), 0, st, a); });
    proj[0] = L_INP_F_1;
  }
  void pre() {
    long nt = 0;                                      // upper bound: the kernel reads the real counts on the device
    for (int k = 1; k <= L; ++k) nt += (((long)B * h->N[k] + 31) / 32) * 2;
    const PreAllArgs a = pre_args();
    const size_t lds = (h->bf3 ? (size_t)PRE_LDS_FLOATS : (size_t)PackPreFwd::FLOATS + PackPreBwd::FLOATS) * 4;
    void (*kern)(PreAllArgs) = h->bf3 ? k_pre<true> : k_pre<false>;
    lz.run(PC_PRE, [&] { hipLaunchKernelGGL(kern, dim3(mlp_grid(h, nt / 8)), dim3(PRE_WAVES * 64), lds, st, a); });
  }
  void pre_inp() {
    const long G = (long)B * h->N[0];
    const TileMap tm = bwd_map(h, 0);
    const long nt = map_tiles(tm, B);
    PreArgs a{h->d_pack[PK_PRE_INP], in->lb[0], in->ub[0], nullptr, nullptr, nullptr, nullptr, ws + w.Q, G, nt, h->N[0], 1,
              to_dtm(tm), nullptr, nullptr};
    lz.run(PC_PRE_INP, [&] { hipLaunchKernelGGL(k_pre_inp, dim3(mlp_grid(h, nt)), dim3(WG_MLP), PackPreInp::FLOATS * 4, st, a); });
  }

  // ---- phase A: aggregates ----
  // round 0's first forward gather computes the input embedding itself (no mu[0] rows: Plan::embed_in_gather)
  bool embed_src(int k) const { return k == 1 && p.embed_in_gather && proj[0] == L_INP_F_1; }
  // a gather over conv edge table `d` into layer k; sparse: behind a ReLU layer (src_layer), skipping the (zero) rows of that
  // layer's dead nodes and producing the bias sums in `sout` on the way
  GArgs gather_args(const DevGather& d, int k, const float* src, bool scored, bool sparse, int src_layer, float* sout) const {
    return GArgs{in->lb[k], in->ub[k], in->mask, src, nb, map_tiles(d.g.tm, B), scored ? 1 : 0, h->R, roff[k], to_dtm(d.g.tm), to_dg(d, h->d_zero.get()),
                 EmbedSrc{in->lb[0], in->x_lp, in->ub[0], h->d_pack[PK_EMBED]}, sparse ? in->lb[src_layer] : nullptr,
                 sparse ? in->ub[src_layer] : nullptr, sparse && w.bits ? reinterpret_cast<const unsigned*>(ws + w.lbits[src_layer]) : nullptr,
                 sparse ? sout : nullptr};
  }
  void gather(const DevGather& d, int k, const float* src, bool scored, bool embed, int src_layer, float* sout) {   // MFMA
    const bool sparse = !embed && src_layer >= 1;
    const GArgs a = gather_args(d, k, src, scored, sparse, src_layer, sout);
    const size_t lds = gather_lds_bytes(d, 0) + (sparse ? sparse_tab_bytes(d) : 0) + (d.g.lanes == 16 ? 16 + (size_t)WAVES_MLP * STAGE16_FLOATS * 4 : 0);
    constexpr int kGatherOcc = 2;     // workgroups per CU (k_gather's launch bounds; its LDS footprint is only the tap matrix)
    long grid = (a.ntiles + WAVES_MLP - 1) / WAVES_MLP;
    if (grid > (long)h->n_cu * kGatherOcc) grid = (long)h->n_cu * kGatherOcc;
    const bool block = !sparse && (d.g.block & (embed ? 2 : 1));      // (a block-form edge: see gnnb_pack.h blocktap_ok)
    void (*kern)(GArgs) = d.g.lanes == 16 ? (embed ? (block ? k_gather16<true, false, true> : k_gather16<true>) : sparse ? k_gather16<false, true>
                                                    : (block ? k_gather16<false, false, true> : k_gather16<false>))
                                          : (embed ? k_gather<true> : sparse ? k_gather<false, true> : k_gather<false>);
    lz.run(PC_GATHER, [&] { hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(WG_MLP), lds, st, a); });
  }
  // nb <- A_e src (forward) or A_e^T src (transposed) over edge e without MFMA gather tables: the VALU conv kernels (the transposed
  // conv divided by the tap count when `normalise`), or for a Linear edge one workgroup per sample with the source rows in LDS
  // where they fit (dense_lds), else the per-tile kernel
  void edge_agg(int ei, bool tr, const float* src, int normalise) {
    const Edge& e = h->edges[ei];
    const DevEdge& de = h->dev[ei];
    if (e.kind == 0) {
      const ConvArgs a{src, nb, tr ? de.w_bwd.get() : de.w_fwd.get(), B, e.c_in, e.h_in, e.w_in, e.c_out, e.h_out, e.w_out, e.kh, e.kw, e.stride, e.pad, normalise};
      void (*kern)(ConvArgs) = tr ? kConvT[conv_channel_form(e.c_in)] : kConvFwd[conv_channel_form(e.c_out)];
      const long waves = tr ? (long)B * e.h_in * e.w_in : (long)B * e.h_out * e.w_out;      // one wave per node of the output side
      lz.run(tr ? PC_CONVT_BWD : PC_CONV_FWD, [&] { hipLaunchKernelGGL(kern, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, st, a); });
      return;
    }
    const float* At = tr ? de.w_bwd.get() : de.w_fwd.get();
    const int Ks = tr ? e.n_out : e.n_in, M = tr ? e.n_in : e.n_out, ld = tr ? de.ld_bwd : de.ld_fwd, MT = tr ? de.mt_bwd : de.mt_fwd;
    if (h->dense_lds && (tr ? de.kpad_bwd <= 128 : de.mt_fwd <= 4)) {
      const DenseLArgs a{At, src, nb, B, Ks, M, ld, MT, tr ? de.kpad_bwd : de.kpad_fwd};
      void (*kern)(DenseLArgs) = tr ? k_dense_bwd_lds : k_dense_fwd_lds;
      lz.run(PC_DENSE_AGG, [&] { hipLaunchKernelGGL(kern, dim3(B), dim3(512), 0, st, a); });
      return;
    }
    const DenseArgs a{At, src, nb, h->d_zero.get(), B, Ks, M, ld, MT, tr ? de.ksq_bwd : de.ksq_fwd};
    const long tiles = (long)B * MT;
    void (*kern)(DenseArgs) = kDenseAgg[Ks >= 512 ? 0 : 1];
    lz.run(PC_DENSE_AGG, [&] { hipLaunchKernelGGL(kern, dim3((unsigned)(Ks >= 512 ? tiles : (tiles + 3) / 4)), dim3(256), 0, st, a); });
  }
  void agg_fwd(int k) {              // nb <- A_k mu[k-1]
    if (h->gf[k].ok) gather(h->gf[k], k, mu(k - 1), false, embed_src(k), k - 1, ws + w.sf[k]);
    else edge_agg(k, false, mu(k - 1), 0);
  }
  // the scored gather of the restricted last step over edge k + 1 into layer k (k_gather_scored, k_scored_tail)
  GSArgs scored_gather_args(int k, float* out, float* sout) const {
    const Edge& e = h->edges[k + 1];
    return GSArgs{ilist(w.score[k]), cnt + 4 * k + 2, mu(k + 1), h->dev[k + 1].w_bwd.get(), in->lb[k + 1], in->ub[k + 1], out, sout,
                  h->N[k], e.c_in, e.h_in, e.w_in, e.c_out, e.h_out, e.w_out, e.kh, e.kw, e.stride, e.pad, 1};
  }
  void agg_bwd(int k, bool scored) {   // nb <- A_{k+1}^T mu[k+1]  (k+1 <= L), divided by the tap count above the input layer
    if (k >= 1 && h->gb[k + 1].ok) {
      if (scored && gs_window_ok(h->edges[k + 1])) {
        // the restricted last step as three kernels (tail_max_b = 0; the default is k_scored_tail): one wave per scored node instead of
        // every tile that holds one (k_gather_scored).  Windows up to GS_SLOT_LIMIT source nodes (base, 64 slots: 31 vs 38 us for the tile
        // gather; deep 18 vs 38; wide, 128 slots: 116 vs 99 -- kept on the list-driven form all the same, so that this path and
        // k_scored_tail evaluate a scored node's aggregate with the same arithmetic)
        const GSArgs a = scored_gather_args(k, nb, ws + w.sb[k]);
        lz.run(PC_GATHER, [&] { hipLaunchKernelGGL(k_gather_scored, dim3((unsigned)h->n_cu * 4), dim3(GS_WAVES * 64), 0, st, a); });
      } else {
        gather(h->gb[k + 1], k, mu(k + 1), scored, false, k + 1, ws + w.sb[k]);
      }
      return;
    }
    // the input layer (k = 0) aggregates the rows of layer 1 that already went through its 64x64 map (PackPostInp)
    edge_agg(k + 1, true, k == 0 ? rows1_for_input : mu(k + 1), k >= 1 ? 1 : 0);
  }

  // ---- phase B: node MLP over a compacted list of nodes ----
  // post_input: this is the backward update of layer 1 and an input-layer update follows -- the kernel also applies the input
  // update's 64x64 map to its rows (PackPostInp) and writes them to F1; only inspection runs still need the plain rows
  // the arguments of the node update of layer k (shared by k_node_update, the fused k_gather_update, k_top and k_scored_tail)
  UpdArgs upd_args(int k, bool fwd, bool scored, bool post_input) const {
    // the aggregate in `nb` was built from rows whose last Linear is deferred (gnnb_pack.h), except the one k_prop writes
    const int src_proj = fwd ? proj[k - 1] : (k < L ? proj[k + 1] : -1);
    int pack = PK_UPD_BWD;
    const float* sarr = nullptr;
    int smod = 0;
    if (fwd) {
      pack = src_proj == L_INP_F_1 ? PK_UPD_FWD_E : (src_proj == L_INP_B2_2 ? PK_UPD_FWD_I : PK_UPD_FWD_F);
      sarr = ws + w.sf[k];
      if (k == 1 && p.s1_table) { sarr = h->d_s1.get(); smod = h->N[1]; }      // the input layer is all live: one table for every sample
    } else if (k < L) {
      pack = PK_UPD_BWD_B;
      sarr = ws + w.sb[k];
    }
    // normal: list0 = live non-ambiguous nodes (short chain), list1 = ambiguous nodes; restricted: the scored nodes, general chain
    UpdArgs a{h->d_pack[pack], in->lb[k], in->ub[k], nb, ws + (fwd ? w.Pf[k] : w.Pb[k]), (post_input && !p.debug_full) ? nullptr : mu(k), status,
              ilist(w.live[k]), cnt + 4 * k + (scored ? 3 : 0), ilist(scored ? w.score[k] : w.amb[k]), cnt + 4 * k + (scored ? 2 : 1), sarr, smod,
              post_input ? rows1_for_input : nullptr, nullptr};
    a.wp = h->d_pack[PK_POST_INP] + (h->bf3 ? (h->gb[1].ok ? PackPostInp::WPG3 : PackPostInp::WPN3) : (h->gb[1].ok ? PackPostInp::WPG : PackPostInp::WPN));
    return a;
  }
  void node_update(int k, bool fwd, bool scored, bool post_input) {
    static void (*const kern[2][2][2])(UpdArgs) = {      // [bf3][deferred][post_input]
        {{k_node_update<8, false>, k_node_update<8, false, true>}, {k_node_update<8, true>, k_node_update<8, true, true>}},
        {{k_node_update<12, false, false, true>, k_node_update<12, false, true, true>},
         {k_node_update<12, true, false, true>, k_node_update<12, true, true, true>}}};
    const long nt = ((long)B * h->N[k] + 31) / 32;
    const UpdArgs a = upd_args(k, fwd, scored, post_input);
    const bool bf3 = h->bf3, deferred = a.sarr != nullptr;
    const int wv = bf3 ? 12 : 8;  // waves per workgroup (one workgroup per CU shares the LDS weights)
    const size_t ldsb = bf3 ? (size_t)(PackUpdL3::FLOATS + (post_input ? 6144 : 0)) * 4 : (size_t)(PackUpd::FLOATS + (post_input ? 4096 : 0)) * 4;
    long grid = (nt + wv - 1) / wv;
    if (grid > h->n_cu) grid = h->n_cu;
    void (*k_upd)(UpdArgs) = kern[bf3][deferred][post_input];
    lz.run(PC_NODE_UPDATE, [&] { hipLaunchKernelGGL(k_upd, dim3((unsigned)grid), dim3(wv * 64), ldsb, st, a); });
    proj[k] = fwd ? L_FC4_2 : L_BC4_1;
  }
  // One half-pass over a conv edge as ONE kernel (k_gather_update): the gather of edge k (forward) / k + 1 (transposed) and the
  // node update of layer k, the aggregate staying in registers.  Returns false where the two-kernel path has to run: inspection
  // runs, the restricted last step (every node it updates takes the general chain), gathers without the sparse walk behind a
  // ReLU layer, tile forms the fused kernel is not built for, tables that do not fit beside the weights in LDS.
  bool fused_halfpass(int k, bool fwd, bool post_input) {
    if (p.debug_full || (!fwd && k >= L)) return false;
    const DevGather& d = fwd ? h->gf[k] : h->gb[k + 1];
    const int src_layer = fwd ? k - 1 : k + 1;
    const bool embed = fwd && embed_src(k);
    if (!fusedq_ok(h, d, src_layer, embed, post_input)) return false;
    const bool sparse = !embed && src_layer >= 1;
    FArgs a{};
    a.g = gather_args(d, k, fwd ? mu(k - 1) : mu(k + 1), false, sparse, src_layer, fwd ? ws + w.sf[k] : ws + w.sb[k]);
    a.u = upd_args(k, fwd, false, post_input);
    a.sw_from_gather = sparse ? 1 : 0;
    a.qtiles = fusedq_qtiles(d, sparse, post_input);
    const size_t ldsq = fusedq_lds_bytes(d, sparse, post_input, a.qtiles);
    const bool block = !sparse && (d.g.block & (embed ? 2 : 1));
    a.npairs = block ? (long)B * pairs_per_sample(d.g.tm) : 0;      // the block-form kernels deal row pairs, not tiles, to their gather waves
    const long nrounds = ((block ? a.npairs : a.g.ntiles) + QG_WAVES - 1) / QG_WAVES;
    // a sparse table build reads the source layer's live bitmap where a sample's bits fit one register per lane (BitsLive), else its bounds
    const bool bits = sparse && w.bits && livebits_ok(d.g.Ns) && d.g.Ns == h->N[src_layer];
    void (*kern)(FArgs) = d.g.lanes == 16 ? (embed ? (block ? k_gather_update_q<16, 2, false, true> : k_gather_update_q<16, 2, false>)
                                                    : sparse ? (bits ? k_gather_update_q<16, 3, false> : k_gather_update_q<16, 1, false>)
                                                    : (block ? k_gather_update_q<16, 0, false, true> : k_gather_update_q<16, 0, false>))
                                          : (post_input ? (bits ? k_gather_update_q<32, 3, true> : k_gather_update_q<32, 1, true>)
                                                        : (bits ? k_gather_update_q<32, 3, false> : k_gather_update_q<32, 1, false>));
    const dim3 g((unsigned)std::max<long>(1, std::min<long>(nrounds, h->n_cu))), b((QG_WAVES + QC_WAVES) * 64);
    lz.run(PC_GATHER_UPDATE, [&] { hipLaunchKernelGGL(kern, g, b, ldsq, st, a); });
    proj[k] = fwd ? L_FC4_2 : L_BC4_1;
    return true;
  }
  void halfpass(int k, bool fwd, bool scored, bool post_input) {      // phase A + phase B of layer k
    if (!scored && fused_halfpass(k, fwd, post_input)) return;
    if (fwd) agg_fwd(k);
    else agg_bwd(k, scored);
    node_update(k, fwd, scored, post_input);
  }
  void update_input() {
    proj[0] = L_INP_B2_2;
    if (h->gb[1].ok) {
      const DevGather& d = h->gb[1];
      const long nt = map_tiles(d.g.tm, B);
      // the sparse walk over the live rows of layer 1, which also yields the bias sums (s_from_gather)
      GIArgs a{h->d_pack[PK_PRE_INP], h->d_pack[PK_UPD_INP], in->lb[0], in->ub[0], rows1_for_input, ws + w.sb[0], mu(0), nt, to_dtm(d.g.tm), to_dg(d, h->d_zero.get()),
               in->lb[1], in->ub[1], 1};
      const size_t lds = gather_lds_bytes(d, PackUpdInp::FLOATS + PackPreInp::FLOATS) + 8 + (size_t)WAVES_MLP * (2 * d.g.K2 + 32) * 8;
      constexpr int kGiuOcc = 2;        // workgroups per CU (<= 128 VGPRs: two 8-wave workgroups fit)
      long giu_grid = (nt + WAVES_MLP - 1) / WAVES_MLP;
      if (giu_grid > (long)h->n_cu * kGiuOcc) giu_grid = (long)h->n_cu * kGiuOcc;
      void (*kern)(GIArgs) = h->bf3 ? k_gather_input_update<true, true> : k_gather_input_update<true, false>;
      lz.run(PC_GATHER_INPUT, [&] { hipLaunchKernelGGL(kern, dim3(giu_grid), dim3(WG_MLP), lds, st, a); });
      return;
    }
    agg_bwd(0, false);
    const long G = (long)B * h->N[0], nt = (G + 31) / 32;
    UpdInpArgs a{h->d_pack[PK_UPD_INP], nb, ws + w.Q, ws + w.sb[0], mu(0), G, nt};
    lz.run(PC_INPUT_UPDATE, [&] { hipLaunchKernelGGL(k_input_update, dim3(mlp_grid(h, nt)), dim3(WG_MLP), PackUpdInp::FLOATS * 4, st, a); });
  }

  // ---- the top of the network ----
  // k_top: the forward half-pass of layer L, the property node and the backward half-pass of layer L in one launch, the aggregate of
  // layer L-1 left in `nb` (and with Plan::top_upd the backward update of layer L-1 done as well)
  void top() {
    const Edge& e = h->edges[L];
    const DevEdge& de = h->dev[L];
    TopArgs a{};
    a.df = DenseLArgs{de.w_fwd.get(), mu(L - 1), nullptr, B, e.n_in, e.n_out, de.ld_fwd, de.mt_fwd, de.kpad_fwd};
    a.db = DenseLArgs{de.w_bwd.get(), nullptr, nb, B, e.n_out, e.n_in, de.ld_bwd, de.mt_bwd, de.kpad_bwd};
    a.pack_f = h->d_pack[PK_UPD_FWD_F]; a.pack_b = h->d_pack[PK_UPD_BWD]; a.pack_p = h->d_pack[PK_PROP];
    a.Pf = ws + w.Pf[L]; a.Pb = ws + w.Pb[L];
    a.sf = p.top_s_fwd ? nullptr : ws + w.sf[L];              // null: F1 walks exactly the live rows of layer L-1 and sums its weights itself
    a.sb_out = p.top_s_bwd ? ws + w.sb[L - 1] : nullptr;
    a.lb = in->lb[L]; a.ub = in->ub[L];
    a.lbm = in->lb[L - 1]; a.ubm = in->ub[L - 1];
    a.prop_w = in->prop_w; a.prop_b = in->prop_b; a.lbK = in->lb[K]; a.ubK = in->ub[K]; a.z_out = in->primal[in->n_primal - 1];
    a.mu_prop = mu(K); a.mu = mu(L); a.status = status; a.N = h->N[L];
    a.xbuf = ws + w.topx; a.xflag = reinterpret_cast<int*>(ws + w.topflag); a.xbase = top_launches * 2 * p.S;
    a.fuse_um = p.top_upd ? 1 : 0;
    if (p.top_upd) a.um = upd_args(L - 1, false, false, false);
    ++top_launches;
    void (*kern)(TopArgs) = p.S == 4 ? k_top<1> : p.S == 2 ? k_top<2> : k_top<4>;
    lz.run(PC_TOP, [&] { hipLaunchKernelGGL(kern, dim3(B * p.S), dim3(512), TOP_LDS_FLOATS * 4, st, a); });
    proj[L] = L_BC4_1;
  }
  // the property node (graph_conv.py:194-210); the backward sweep starts with the edge from it, whose aggregate the same kernel writes
  void prop(bool bwd_follows) {
    PropArgs a{h->d_pack[PK_PROP], mu(L), in->prop_w, in->prop_b, in->lb[K], in->ub[K], in->primal[in->n_primal - 1], mu(K),
               bwd_follows ? nb : nullptr, B, h->N[L], in->lb[L], in->ub[L]};
    lz.run(PC_PROP_FWD, [&] { hipLaunchKernelGGL(k_prop, dim3(B), dim3(256), 0, st, a); });
  }

  // scores (graph_conv.py:442-450) and decision (graph_score.py:41-47); with Plan::tail the restricted last step (scored gather +
  // node update of layer 1) and the score head are ONE launch, k_scored_tail (tail_max_b = 0: k_gather_scored, k_node_update, k_score)
  void score() {
    ScoreArgs a{};
    a.best = best(); a.done = done_ctr(); a.dec = decisions; a.B = B; a.n_relu = L;
    a.pack = h->d_pack[proj[1] == L_FC4_2 ? PK_SCORE_F : PK_SCORE_B]; a.scores = scores; a.L = L; a.R = h->R; a.cnt = cnt + 4; a.cnt_all = cnt;
    long nt = 0;
    for (int k = 1; k <= L; ++k) {
      const int i = k - 1;
      a.mu[i] = mu(k); a.list[i] = ilist(w.score[k]); a.N[i] = h->N[k]; a.off[i] = roff[k];
      a.lb[i] = in->lb[k]; a.ub[i] = in->ub[k];
      nt += ((long)B * h->N[k] + 31) / 32;
      a.cum[k - 1] = roff[k] + h->N[k];
    }
    if (!p.tail) {
      lz.run(PC_SCORE, [&] { hipLaunchKernelGGL(k_score, dim3(mlp_grid(h, nt / 4)), dim3(WG_MLP), PackScore::FLOATS * 4, st, a); });
      return;
    }
    TailArgs tail{};
    tail.g = scored_gather_args(1, nullptr, nullptr);
    tail.f.u = upd_args(1, false, true, false);
    tail.f.sw_from_gather = 1;
    tail.s = a;
    const int grid = (int)std::min<long>(h->n_cu, std::max<long>(1, ((long)B * h->N[1] + 15) / 16));
    const int nslots = gs_slots(h->edges[2]);
    tail.sp = tail_slots_pad(nslots);
    lz.run(PC_SCORE, [&] { hipLaunchKernelGGL(k_scored_tail, dim3(grid), dim3(TAIL_WAVES * 64), tail_lds_bytes(nslots), st, tail); });
  }
};

extern "C" int gnnb_forward(gnnb_t* h, const gnnb_batch* in, int B, float* scores, int32_t* decisions, int32_t* status,
                            void* workspace, size_t workspace_bytes, void* stream) {
  if (!h || !in || !scores || !decisions || !status || !workspace) return fail(GNNB_E_INVALID, "gnnb_forward: null argument");
  if (!h->bound) return fail(GNNB_E_STATE, "gnnb_forward: call gnnb_bind_network first");
  if (int rc = refuse_zero_taps(h, "gnnb_forward")) return rc;
  if (int rc = refuse_batch(h, in, B, kNeedsForward, "gnnb_forward")) return rc;
  const int L = (int)h->N.size() - 2;
  const WsLayout w = ws_layout(h, B);
  if (workspace_bytes < w.total * sizeof(float))
    return fail(GNNB_E_NOMEM, "gnnb_forward: workspace %zu bytes < required %zu", workspace_bytes, w.total * sizeof(float));
  hipStream_t st = (hipStream_t)stream;
  // the counters' control block of this workspace (see gnnb_handle::d_ctl); a workspace seen for the first time (or after a failed
  // call) gets a freshly zeroed one -- an async memset on the stream, the only time anything but kernels is enqueued
  int slot = -1;
  for (int i = 0; i < 8; ++i)
    if (h->ctl_ws[i] == workspace) slot = i;
  if (slot < 0) {
    slot = 0;
    for (int i = 1; i < 8; ++i)
      if (h->ctl_age[i] < h->ctl_age[slot]) slot = i;
    HIPCHK(hipMemsetAsync(h->d_ctl.get() + 64 * slot, 0, 64 * sizeof(int), st));
    h->ctl_ws[slot] = workspace;
  }
  h->ctl_age[slot] = ++h->ctl_clock;

  const Plan p = make_plan(h, B, h->halfpass_limit);
  Forward f(h, in, B, p, w, workspace, scores, decisions, status, st, h->d_ctl.get() + 64 * slot);
  f.classify();
  f.livesum();
  f.input_embedding();
  if (!p.cls_pre) f.pre();
  if (p.need_inp) f.pre_inp();
  // T rounds (graph_conv.py:107-388): forward sweep up to layer last_fwd, then k_top (F1 .. B2: both half-passes of layer L) or
  // k_prop (the property node); either leaves the aggregate of layer last_fwd in `nb` for the backward sweep, which runs in
  // Gauss-Seidel order (layer k reads the already-updated mu[k+1]).  A half-pass limit (inspection; no k_top) may stop after the
  // forward sweep.
  const int last_fwd = p.top_fused ? L - 1 : L;
  int done = 0;
  for (int t = 0; t < h->T && done < p.limit; ++t) {
    const bool last_round = t == h->T - 1;
    for (int k = 1; k <= last_fwd; ++k) f.halfpass(k, true, false, false);
    if (p.top_fused) f.top();
    else f.prop(done + 1 < p.limit);
    if (++done >= p.limit) break;
    for (int k = last_fwd; k >= 1; --k) {
      // after the last backward step mu[1] is only read by the score head, i.e. at the scored nodes
      const bool scored = !p.debug_full && last_round && k == 1, post_input = k == 1 && (!last_round || p.debug_full);
      if (k == last_fwd && p.top_upd) f.proj[k] = L_BC4_1;            // done inside k_top
      else if (k == last_fwd) f.node_update(k, false, scored, post_input);      // its aggregate is already in `nb`
      else if (scored && p.tail) f.proj[k] = L_BC4_1;                  // k_scored_tail, launched with the score head
      else f.halfpass(k, false, scored, post_input);
    }
    // input layer (:360-385): its last-round result is never read, so it only runs when another round follows
    if (!last_round || p.debug_full) f.update_input();
    ++done;
  }
  f.score();
  for (int k = 0; k < MAXL + 2; ++k) h->last_proj[k] = f.proj[k];      // inspection (gnnb_mu_projection); one handle per thread
  if (f.lz.rc) h->ctl_ws[slot] = nullptr;          // a launch failed: the counters may be left non-zero, the block is re-zeroed on its next use
  return f.lz.rc;
}

// gnnb_forward for HOST inputs -- the reference's own call pattern: one or two subproblems per decision, every tensor a CPU
// tensor (graph_score.py:26-30 moves them with ~14 .cuda() calls).  All inputs the forward reads are packed into one pinned
// buffer (256-B aligned slots) and cross PCIe as ONE copy; the forward runs on `stream`; decisions, status and (optionally) the
// padded scores come back in one pinned block; the call returns after synchronising the stream.  Buffers live in the handle.
extern "C" int gnnb_forward_host(gnnb_t* h, const gnnb_batch* in, int B, float* scores, int32_t* decisions, int32_t* status, void* stream) {
  if (!h || !in || !decisions || !status) return fail(GNNB_E_INVALID, "gnnb_forward_host: null argument");
  if (!h->bound) return fail(GNNB_E_STATE, "gnnb_forward_host: call gnnb_bind_network first");
  if (int rc = refuse_zero_taps(h, "gnnb_forward_host")) return rc;
  if (int rc = refuse_batch(h, in, B, kNeedsForwardHost, "gnnb_forward_host")) return rc;
  const int K = (int)h->N.size() - 1, L = K - 1, R = h->R;
  hipStream_t st = (hipStream_t)stream;
  // ---- slots: (host pointer, floats); primals the forward never reads are not transferred
  struct Slot { const float* src; size_t n, off; };
  std::vector<Slot> slots;
  size_t total = 0;
  auto add = [&](const float* p, size_t n) { slots.push_back(Slot{p, n, total}); total += (n + 63) & ~(size_t)63; return slots.size() - 1; };
  std::vector<size_t> i_lb(K + 1), i_ub(K + 1), i_dual(L), i_prim(in->n_primal, (size_t)-1);
  for (int k = 0; k <= K; ++k) { i_lb[k] = add(in->lb[k], (size_t)B * h->N[k]); i_ub[k] = add(in->ub[k], (size_t)B * h->N[k]); }
  for (int k = 0; k < L; ++k) i_dual[k] = add(in->dual[k], (size_t)B * h->N[k + 1] * 3);
  for (int k = 1; k <= L; ++k)
    for (int m : {h->relu_q[k] - 1, h->relu_q[k]})
      if (i_prim[m] == (size_t)-1) i_prim[m] = add(in->primal[m], (size_t)B * h->N[k]);
  if (i_prim[in->n_primal - 1] == (size_t)-1) i_prim[in->n_primal - 1] = add(in->primal[in->n_primal - 1], (size_t)B);
  const size_t i_x = add(in->x_lp, (size_t)B * h->N[0]), i_pw = add(in->prop_w, (size_t)B * h->N[L]), i_pb = add(in->prop_b, (size_t)B);
  const size_t i_mask = add(in->mask, (size_t)B * R);
  for (const Slot& sl : slots) {
    // these are read by memcpy on the host: device memory here is a caller bug (e.g. data_ptr() of a `.cuda()` tensor), refused
    // rather than dereferenced.  ~0.2 us per pointer: the runtime's allocation map, no driver call
    hipPointerAttribute_t at{};
    if (hipPointerGetAttributes(&at, sl.src) != hipSuccess) { (void)hipGetLastError(); continue; }      // plain host memory
    if (at.type == hipMemoryTypeDevice) return fail(GNNB_E_INVALID, "gnnb_forward_host: an input pointer is device memory; this entry point takes host pointers (gnnb_forward takes device pointers)");
  }
  // ---- buffers
  HIPCHK(h->hs_pinned.grow(total));
  HIPCHK(h->hs_dev.grow(total));
  HIPCHK(h->hs_ws.grow(gnnb_workspace_bytes(h, B)));
  HIPCHK(h->hs_scores.grow((size_t)B * R));
  HIPCHK(h->hs_dec.grow((size_t)B * 2 + 1));          // decisions, then the status word
  HIPCHK(h->hs_out_pinned.grow((size_t)B * R + (size_t)B * 2 + 1));
  // ---- stage, one transfer, forward
  // staging: one memcpy per input tensor; big batches (36.5 MB at base B = 256: 2.3 ms on one thread) are split over the handle's helper threads
  if (total * sizeof(float) < (size_t)4 << 20) {
    for (const Slot& sl : slots) memcpy(h->hs_pinned.get() + sl.off, sl.src, sl.n * sizeof(float));
  } else {
    const size_t chunk = (size_t)1 << 18;                 // floats (1 MB) per work item
    std::vector<std::pair<size_t, size_t>> items;         // (slot, first float)
    for (size_t i = 0; i < slots.size(); ++i)
      for (size_t o = 0; o < slots[i].n; o += chunk) items.emplace_back(i, o);
    std::atomic<size_t> next{0};
    work_pool(h).run([&]() {
      for (size_t it = next.fetch_add(1); it < items.size(); it = next.fetch_add(1)) {
        const Slot& sl = slots[items[it].first];
        const size_t o = items[it].second, n = std::min(chunk, sl.n - o);
        memcpy(h->hs_pinned.get() + sl.off + o, sl.src + o, n * sizeof(float));
      }
    });
  }
  float* const dev = h->hs_dev.get();
  HIPCHK(hipMemcpyAsync(dev, h->hs_pinned.get(), total * sizeof(float), hipMemcpyHostToDevice, st));
  std::vector<const float*> lb(K + 1), ub(K + 1), dual(L), prim(in->n_primal);
  for (int k = 0; k <= K; ++k) { lb[k] = dev + slots[i_lb[k]].off; ub[k] = dev + slots[i_ub[k]].off; }
  for (int k = 0; k < L; ++k) dual[k] = dev + slots[i_dual[k]].off;
  for (int m = 0; m < in->n_primal; ++m) prim[m] = i_prim[m] == (size_t)-1 ? dev : dev + slots[i_prim[m]].off;   // (unread ones: any valid pointer)
  gnnb_batch dv{lb.data(), ub.data(), dual.data(), prim.data(), dev + slots[i_x].off, dev + slots[i_pw].off,
                dev + slots[i_pb].off, dev + slots[i_mask].off, in->n_graph, in->n_relu, in->n_primal};
  int32_t* const d_dec = h->hs_dec.get();
  if (int rc = gnnb_forward(h, &dv, B, h->hs_scores.get(), d_dec, d_dec + (size_t)B * 2, h->hs_ws.get(), h->hs_ws.size(), stream)) return rc;
  int32_t* out_i = reinterpret_cast<int32_t*>(h->hs_out_pinned.get());
  HIPCHK(hipMemcpyAsync(out_i, d_dec, ((size_t)B * 2 + 1) * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  float* out_s = h->hs_out_pinned.get() + (size_t)B * 2 + 1;
  if (scores) HIPCHK(hipMemcpyAsync(out_s, h->hs_scores.get(), (size_t)B * R * sizeof(float), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  memcpy(decisions, out_i, (size_t)B * 2 * sizeof(int32_t));
  *status = out_i[(size_t)B * 2];
  if (scores) memcpy(scores, out_s, (size_t)B * R * sizeof(float));
  return GNNB_OK;
}

// ---- host-fed batches: compact records of the ambiguous nodes instead of whole dual / primal tensors (include/gnnb.h) --------------------
extern "C" size_t gnnb_amb_records_bytes(const gnnb_t* h, int B) {
  if (!h || !h->bound || B < 1) return 0;
  const int L = (int)h->N.size() - 2;
  size_t words = 16 + (size_t)((B + 3) & ~3);
  for (int k = 1; k <= L; ++k) words += (size_t)AMBREC_WORDS * B * h->N[k];
  return words * 4;
}

extern "C" int gnnb_pack_amb_records(const gnnb_t* hc, const gnnb_batch* in, int B, void* dst, size_t cap, size_t* used) {
  gnnb_t* h = const_cast<gnnb_t*>(hc);                  // (the helper threads live in the handle)
  if (!h || !in || !dst || !used) return fail(GNNB_E_INVALID, "gnnb_pack_amb_records: null argument");
  if (!h->bound) return fail(GNNB_E_STATE, "gnnb_pack_amb_records: call gnnb_bind_network first");
  if (int rc = refuse_batch(h, in, B, kNeedsPack, "gnnb_pack_amb_records")) return rc;
  const int L = (int)h->N.size() - 2;
  const size_t zwords = (size_t)((B + 3) & ~3);
  if (cap < (16 + zwords) * 4) return fail(GNNB_E_NOMEM, "gnnb_pack_amb_records: buffer of %zu bytes is too small", cap);
  const size_t max_rec = (cap / 4 - 16 - zwords) / AMBREC_WORDS;
  // ONE pass: work items = contiguous node ranges of a layer; a thread collects the records of its range in a local block and copies
  // the block behind an atomic cursor.  The order of the records in the image is whatever the threads make it: the scatter does not care.
  struct Item { int k; long lo, hi; };
  std::vector<Item> items;
  const long chunk = 1L << 15;
  for (int k = 1; k <= L; ++k) {
    const long G = (long)B * h->N[k];
    for (long lo = 0; lo < G; lo += chunk) items.push_back(Item{k, lo, std::min(G, lo + chunk)});
  }
  int32_t* img = reinterpret_cast<int32_t*>(dst);
  int32_t* recs = img + 16;
  std::atomic<size_t> next{0}, cursor{0};
  std::atomic<int> overflow{0};
  const std::function<void()> work = [&]() {
    constexpr int BLK = 1024;
    int32_t local[BLK * AMBREC_WORDS];
    for (size_t it = next.fetch_add(1); it < items.size(); it = next.fetch_add(1)) {
      const Item& w = items[it];
      const int k = w.k;
      const ReluRows r = relu_rows(*h, *in, B, k);
      const float *lb = r.lb, *ub = r.ub, *du = r.dual, *zp = r.z_pre, *zq = r.z_post;
      int n = 0;
      auto flush = [&]() {
        if (!n) return;
        const size_t at = cursor.fetch_add((size_t)n);
        if (at + n > max_rec) overflow.store(1);
        else memcpy(recs + at * AMBREC_WORDS, local, (size_t)n * AMBREC_WORDS * 4);
        n = 0;
      };
      for (long g = w.lo; g < w.hi; ++g) {
        if (!(lb[g] < 0.0f && ub[g] > 0.0f)) continue;
        int32_t* r = local + n * AMBREC_WORDS;
        r[0] = k - 1; r[1] = (int32_t)g;
        memcpy(r + 2, du + g * 3 + 1, 8);
        memcpy(r + 4, zp + g, 4);
        memcpy(r + 5, zq + g, 4);
        if (++n == BLK) flush();
      }
      flush();
    }
  };
  if (items.size() >= 8) work_pool(h).run(work);
  else work();
  const size_t total = cursor.load();
  if (overflow.load() || total > max_rec) return fail(GNNB_E_NOMEM, "gnnb_pack_amb_records: %zu records do not fit a buffer of %zu bytes", total, cap);
  memset(img, 0, 64);
  img[0] = AMBREC_MAGIC; img[1] = L; img[2] = (int32_t)total; img[3] = B;
  memcpy(recs + total * AMBREC_WORDS, in->primal[in->n_primal - 1], (size_t)B * sizeof(float));
  *used = (16 + total * AMBREC_WORDS + zwords) * 4;
  return GNNB_OK;
}

extern "C" int gnnb_scatter_amb_records(gnnb_t* h, const void* dev_image, int B, float* const* dual, int n_relu, float* const* primal, int n_primal,
                                        int32_t* status, void* stream) {
  if (!h || !dev_image || !dual || !primal) return fail(GNNB_E_INVALID, "gnnb_scatter_amb_records: null argument");
  if (!h->bound) return fail(GNNB_E_STATE, "gnnb_scatter_amb_records: call gnnb_bind_network first");
  const int L = (int)h->N.size() - 2;
  if (B < 1 || L > MAXL || n_relu != L || n_primal != h->n_fixed + 1) return fail(GNNB_E_INVALID, "gnnb_scatter_amb_records: arrays do not match the bound network");
  ScatterArgs a{};
  a.image = reinterpret_cast<const int*>(dev_image); a.L = L; a.B = B;
  long total = B;
  for (int k = 1; k <= L; ++k) {
    const int q = h->relu_q[k];
    if (!dual[k - 1] || !primal[q - 1] || !primal[q]) return fail(GNNB_E_INVALID, "gnnb_scatter_amb_records: null array (layer %d)", k);
    a.dual[k - 1] = dual[k - 1]; a.z_pre[k - 1] = primal[q - 1]; a.z_post[k - 1] = primal[q];
    a.G[k - 1] = (long)B * h->N[k];
    total += (long)B * h->N[k];                          // (upper bound: the kernel reads the real counts from the image)
  }
  a.max_rec = total - B;
  a.status = status;
  if (!primal[n_primal - 1]) return fail(GNNB_E_INVALID, "gnnb_scatter_amb_records: null primals[-1]");
  a.z_out = primal[n_primal - 1];
  // (grid-stride: sized for an eighth of the nodes being ambiguous, correct for any share)
  hipLaunchKernelGGL(k_scatter_amb, dim3((unsigned)std::min<long>(1024, (total / 8 + 255) / 256 + 1)), dim3(256), 0, (hipStream_t)stream, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(GNNB_E_HIP, "launch of k_scatter_amb failed: %s", hipGetErrorString(e));
  return GNNB_OK;
}

// BaBSR scores of a batch (reference plnn/kw_score_conv.py choose_node_conv :41-113; the decision rule :115-156 stays
// on the host).  lb/ub: HOST tables of n_graph DEVICE pointers exactly as in gnnb_batch; prop_w (B, N_L), mask (B, R),
// scores/intercepts (B, R) device.  Stream-ordered, no allocation.
extern "C" int gnnb_babsr(gnnb_t* h, const float* const* lb, const float* const* ub, int n_graph, const float* prop_w,
                          const float* mask, int B, float* scores, float* intercepts, void* stream) {
  if (!h || !lb || !ub || !prop_w || !mask || !scores || !intercepts) return fail(GNNB_E_INVALID, "gnnb_babsr: null argument");
  if (!h->bound) return fail(GNNB_E_STATE, "gnnb_babsr: call gnnb_bind_network first");
  const int K = (int)h->N.size() - 1, L = K - 1;
  if (n_graph != K + 1 || B < 1) return fail(GNNB_E_INVALID, "gnnb_babsr: %d graph layers given, network has %d", n_graph, K + 1);
  BabsrArgs a{};
  a.L = L; a.R = h->R; a.prop_w = prop_w; a.mask = mask; a.scores = scores; a.icp = intercepts;
  int off = 0, maxN = 0;
  for (int k = 1; k <= L; ++k) {
    const int i = k - 1;
    if (!lb[k] || !ub[k]) return fail(GNNB_E_INVALID, "gnnb_babsr: null bounds pointer for graph layer %d", k);
    a.lb[i] = lb[k]; a.ub[i] = ub[k]; a.bias[i] = h->dev[k].bias.get(); a.N[i] = h->N[k]; a.hw[i] = h->hw[k]; a.off[i] = off;
    off += h->N[k];
    maxN = std::max(maxN, h->N[k]);
    if (k < L) {                              // edge k+1 (between graph layers k and k+1)
      const Edge& e = h->edges[k + 1];
      a.ekind[i] = e.kind; a.ew[i] = h->dev[k + 1].w_bwd.get();
      a.c_in[i] = e.c_in; a.h_in[i] = e.h_in; a.w_in[i] = e.w_in; a.c_out[i] = e.c_out; a.h_out[i] = e.h_out; a.w_out[i] = e.w_out;
      a.kh[i] = e.kh; a.kw[i] = e.kw; a.stride[i] = e.stride; a.pad[i] = e.pad; a.ld[i] = h->dev[k + 1].ld_bwd;
    }
  }
  a.maxN = maxN;
  const size_t lds = (size_t)2 * maxN * sizeof(float);
  if (lds > BABSR_LDS_MAX) {
    int wide = 1;
    for (int k = 2; k <= L; ++k) if (h->N[k] > h->N[wide]) wide = k;
    return fail(GNNB_E_INVALID, "gnnb_babsr: ReLU layer %d of %d nodes needs %zu bytes of LDS for the ratio buffers (%d at most)", wide, maxN, lds,
                BABSR_LDS_MAX);
  }
  hipLaunchKernelGGL(k_babsr, dim3(B), dim3(256), lds, (hipStream_t)stream, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(GNNB_E_HIP, "launch of k_babsr failed: %s", hipGetErrorString(e));
  return GNNB_OK;
}


// ================================================================================================================
// Wong-Kolter intermediate bounds of a batch of BaB domains (gnnb_k_kw.h; lp_producer.py LayerGraphLP.kw_bounds, reference
// plnn/dual_network_linear_approximation.py init_kw_bounds :205-294 / update_kw_bounds :296-451).  The network itself -- sizes, ReLU offsets,
// layer shapes, edge geometry, fp64 weights -- is the handle's KwNet, made by gnnb_bind_network; a call adds only its own pointers.
// ================================================================================================================
struct KwWs { size_t pw, total; };      // byte offsets in the workspace: (d, -d l) pairs at 0, then the fp64 property layers
static KwWs kw_ws_layout(const gnnb_t* h, int B) {
  const int L = (int)h->N.size() - 2;
  KwWs w;
  w.pw = ((size_t)B * h->R * 2 * sizeof(double) + 255) & ~(size_t)255;
  w.total = w.pw + (((size_t)B * (h->N[L] + 1) * sizeof(double) + 255) & ~(size_t)255);
  return w;
}

extern "C" size_t gnnb_kw_workspace_bytes(const gnnb_t* h, int B) {
  if (!h || !h->bound || B < 1) return 0;
  return kw_ws_layout(h, B).total;
}

// What gnnb_kw_bounds and gnnb_dual_ascent check before anything else: the handle, the bound network (1..MAXL ReLU layers, as many graph
// layers as the caller's batch says: n_graph points into it) and the LDS their kernels need for two buffers of the widest ReLU layer.
// *lds: that size in bytes.
static int kw_preflight(const gnnb_t* h, const char* who, const int* n_graph, size_t* lds) {
  if (!h) return fail(GNNB_E_INVALID, "%s: null handle", who);
  if (!h->bound) return fail(GNNB_E_STATE, "%s: call gnnb_bind_network first", who);
  if (!n_graph) return fail(GNNB_E_INVALID, "%s: null batch", who);
  const KwNet& net = h->kw_net;
  if (*n_graph != net.L + 2) return fail(GNNB_E_INVALID, "%s: %d graph layers given, network has %d", who, *n_graph, net.L + 2);
  if (net.L < 1 || net.L > MAXL) return fail(GNNB_E_INVALID, "%s: %d ReLU layers (1..%d)", who, net.L, MAXL);
  *lds = kw_lds_doubles(net.maxNr) * sizeof(double);
  if (*lds > 65536)
    return fail(GNNB_E_INVALID, "%s: a ReLU layer of %d nodes needs %zu bytes of LDS for the dual pass (64 KiB at most)", who, net.maxNr, *lds);
  return GNNB_OK;
}

// Everything gnnb_kw_bounds (and gnnb_kw_tighten, for the same arguments) checks before a launch, and the kernels' arguments
static int kw_make_args(gnnb_t* h, const char* who, const gnnb_kw_batch* in, int B, double* const* lb, double* const* ub, float* const* lb32,
                        float* const* ub32, int32_t* infeasible, void* workspace, size_t workspace_bytes, KwArgs* out, size_t* lds_out) {
  size_t lds = 0;
  if (int rc = kw_preflight(h, who, in ? &in->n_graph : nullptr, &lds)) return rc;
  if (!lb || !ub || !infeasible || !workspace || B < 1 || B > 65535)      // (65535: k_kw_layer's grid is (N_k, B))
    return fail(GNNB_E_INVALID, "%s: null argument or batch size %d outside 1..65535", who, B);
  if (!in->x_lo || !in->x_hi || !in->prop_w || !in->prop_b || !in->mask) return fail(GNNB_E_INVALID, "%s: null input pointer", who);
  if ((in->parent_lb == nullptr) != (in->parent_ub == nullptr) || (in->parent_lb && !in->split_layer))
    return fail(GNNB_E_INVALID, "%s: parent bounds need both tables and split_layer", who);
  if ((lb32 == nullptr) != (ub32 == nullptr)) return fail(GNNB_E_INVALID, "%s: lb32 and ub32 go together", who);
  const KwWs ws = kw_ws_layout(h, B);
  if (workspace_bytes < ws.total) return fail(GNNB_E_NOMEM, "%s: workspace %zu bytes, need %zu", who, workspace_bytes, ws.total);
  KwArgs a{};
  a.net = h->kw_net;
  a.B = B;
  const int L = a.net.L, K = L + 1, NL = a.net.N[L];      // graph layers 0..K, K the property node
  for (int k = 1; k <= K; ++k) {
    if (!lb[k - 1] || !ub[k - 1]) return fail(GNNB_E_INVALID, "%s: null output pointer for graph layer %d", who, k);
    a.lb[k] = lb[k - 1]; a.ub[k] = ub[k - 1];
    if (in->parent_lb) {
      if (!in->parent_lb[k - 1] || !in->parent_ub[k - 1]) return fail(GNNB_E_INVALID, "%s: null parent pointer for graph layer %d", who, k);
      a.plb[k] = in->parent_lb[k - 1]; a.pub[k] = in->parent_ub[k - 1];
    }
  }
  for (int k = 0; k <= K; ++k)
    if (lb32) {
      if (!lb32[k] || !ub32[k]) return fail(GNNB_E_INVALID, "%s: null fp32 output pointer for graph layer %d", who, k);
      a.lb32[k] = lb32[k]; a.ub32[k] = ub32[k];
    }
  a.x_lo = in->x_lo; a.x_hi = in->x_hi; a.prop_w = in->prop_w; a.prop_b = in->prop_b; a.mask = in->mask;
  a.split = in->parent_lb ? in->split_layer : nullptr;
  a.dg = (double*)workspace;
  a.pw = (double*)((char*)workspace + ws.pw);
  KwEdge& P = a.net.e[K];                                 // the property layer: per-domain Linear(N_L, 1), fp64 copy in this call's workspace
  P.w = a.pw; P.bias = a.pw + NL; P.wb = P.bb = NL + 1; P.kind = 1;
  P.n_in = NL; P.n_out = 1;
  a.infeasible = infeasible;
  *out = a;
  *lds_out = lds;
  return GNNB_OK;
}

// graph layers 1..L+1 of one chain (k_kw_flag is the caller's)
static void kw_launch_chain(Launcher& run, const KwArgs& a, size_t lds) {
  hipStream_t st = run.st;
  const int B = a.B, K = a.net.L + 1, NL = a.net.N[a.net.L];
  const int span = std::max(std::max(a.net.N[0], a.net.N[1]), NL + 1);
  const long nthreads = (long)span * B;
  run.run(PC_KW_FIRST, [&] { hipLaunchKernelGGL(k_kw_first, dim3((unsigned)((nthreads + KW_THREADS - 1) / KW_THREADS)), dim3(KW_THREADS), 0, st, a, span); });
  for (int k = 2; k <= K; ++k)
    run.run(PC_KW_LAYER, [&] { hipLaunchKernelGGL(k_kw_layer, dim3(a.net.N[k], B), dim3(KW_THREADS), lds, st, a, k); });
}

extern "C" int gnnb_kw_bounds(gnnb_t* h, const gnnb_kw_batch* in, int B, double* const* lb, double* const* ub, float* const* lb32,
                              float* const* ub32, int32_t* infeasible, void* workspace, size_t workspace_bytes, void* stream) {
  KwArgs a{};
  size_t lds = 0;
  if (int rc = kw_make_args(h, "gnnb_kw_bounds", in, B, lb, ub, lb32, ub32, infeasible, workspace, workspace_bytes, &a, &lds)) return rc;
  hipStream_t st = (hipStream_t)stream;
  Launcher run{h, st};
  kw_launch_chain(run, a, lds);
  run.run(PC_KW_FLAG, [&] { hipLaunchKernelGGL(k_kw_flag, dim3(B), dim3(KW_THREADS), 0, st, a); });
  return run.rc;
}


// ================================================================================================================
// Intermediate bounds tightened by per-node dual ascent (gnnb_k_tighten.h; lp_producer.py LayerGraphLP.kw_bounds(tighten=n); DESIGN.md
// section 7.18)
// ================================================================================================================
struct TightenWs { size_t dg, plo, pup, state, total; int st_off[MAXL + 2], cap[MAXL + 2]; };   // byte offsets (the node flags at 0); per graph layer
static TightenWs tighten_ws_layout(const gnnb_t* h, int B) {                                   // where the state lives and its doubles per node
  const KwNet& net = h->kw_net;
  auto pad = [](size_t n) { return (n + 255) & ~(size_t)255; };
  size_t nodes = 0, spill = 0;
  for (int k = 1; k <= net.L; ++k) nodes += (size_t)net.N[k];
  nodes += 1;                                             // the property node
  TightenWs w{};
  const size_t base = kw_lds_doubles(net.maxNr);
  for (int k = 2; k <= net.L; ++k) {
    const size_t need = tighten_state_doubles(net, k);
    const bool in_lds = (base + need) * sizeof(double) <= 65536;
    w.cap[k] = (int)need;
    w.st_off[k] = in_lds ? (int)base : -1;
    if (!in_lds) spill = std::max(spill, need * (size_t)net.N[k]);
  }
  w.dg = pad((size_t)B * net.R);
  w.plo = w.dg + pad((size_t)B * net.R * 2 * sizeof(double));
  w.pup = w.plo + pad((size_t)B * nodes * sizeof(double));
  w.state = w.pup + pad((size_t)B * nodes * sizeof(double));
  w.total = w.state + pad((size_t)B * spill * sizeof(double));
  return w;
}

extern "C" size_t gnnb_kw_tighten_workspace_bytes(const gnnb_t* h, int B) {
  if (!h || !h->bound || B < 1) return 0;
  return tighten_ws_layout(h, B).total;
}

extern "C" int gnnb_kw_tighten(gnnb_t* h, const gnnb_kw_batch* in, int B, int n_iter, double lr, double* const* lb, double* const* ub,
                               float* const* lb32, float* const* ub32, int32_t* infeasible, int32_t* counts, void* kw_workspace,
                               size_t kw_workspace_bytes, void* workspace, size_t workspace_bytes, void* stream) {
  TightenArgs t{};
  size_t lds = 0;
  if (h && (n_iter < 0 || !(lr > 0.0) || !std::isfinite(lr)))
    return fail(GNNB_E_INVALID, "gnnb_kw_tighten: %d iterations with step %g (at least 0; positive and finite)", n_iter, lr);
  if (int rc = kw_make_args(h, "gnnb_kw_tighten", in, B, lb, ub, lb32, ub32, infeasible, kw_workspace, kw_workspace_bytes, &t.kw, &lds)) return rc;
  if (!workspace) return fail(GNNB_E_INVALID, "gnnb_kw_tighten: null workspace");
  const TightenWs ws = tighten_ws_layout(h, B);
  if (workspace_bytes < ws.total) return fail(GNNB_E_NOMEM, "gnnb_kw_tighten: workspace %zu bytes, need %zu", workspace_bytes, ws.total);
  const KwArgs& a = t.kw;
  const int L = a.net.L, K = L + 1;
  hipStream_t st = (hipStream_t)stream;
  Launcher run{h, st};
  if (n_iter == 0) {                                      // gnnb_kw_bounds, launch for launch
    kw_launch_chain(run, a, lds);
    run.run(PC_KW_FLAG, [&] { hipLaunchKernelGGL(k_kw_flag, dim3(B), dim3(KW_THREADS), 0, st, a); });
    if (counts && !run.rc) HIPCHK(hipMemsetAsync(counts, 0, (size_t)B * 2 * sizeof(int32_t), st));
    return run.rc;
  }
  // the plain chain first, into the workspace: what every layer of the tightened chain is met with
  KwArgs p = a;
  p.dg = (double*)((char*)workspace + ws.dg);
  size_t at = 0;
  for (int k = 1; k <= K; ++k) {
    p.lb[k] = (double*)((char*)workspace + ws.plo) + at;
    p.ub[k] = (double*)((char*)workspace + ws.pup) + at;
    t.plo[k] = p.lb[k]; t.pup[k] = p.ub[k];
    at += (size_t)B * a.net.N[k];
  }
  for (int k = 0; k <= K; ++k) p.lb32[k] = p.ub32[k] = nullptr;
  kw_launch_chain(run, p, lds);
  t.n_iter = n_iter; t.lr = lr;
  t.ran = (int8_t*)workspace;
  t.ws = (double*)((char*)workspace + ws.state);
  t.counts = counts;
  const int span = std::max(std::max(a.net.N[0], a.net.N[1]), a.net.N[L] + 1);
  const long nthreads = (long)span * B;
  run.run(PC_KW_FIRST, [&] { hipLaunchKernelGGL(k_kw_first, dim3((unsigned)((nthreads + KW_THREADS - 1) / KW_THREADS)), dim3(KW_THREADS), 0, st, a, span); });
  for (int k = 2; k <= K; ++k) {
    const unsigned meet = (unsigned)(((long)a.net.N[k] * B + KW_THREADS - 1) / KW_THREADS);
    run.run(PC_KW_LAYER, [&] { hipLaunchKernelGGL(k_kw_layer, dim3(a.net.N[k], B), dim3(KW_THREADS), lds, st, a, k); });
    run.run(PC_KW_LAYER, [&] { hipLaunchKernelGGL(k_kw_meet, dim3(meet), dim3(KW_THREADS), 0, st, t, k); });
    if (k <= L) {
      const size_t tl = lds + (ws.st_off[k] >= 0 ? (size_t)ws.cap[k] * sizeof(double) : 0);
      run.run(PC_KW_LAYER, [&] { hipLaunchKernelGGL(k_kw_tighten, dim3(a.net.N[k], B), dim3(KW_THREADS), tl, st, t, k, ws.st_off[k], ws.cap[k]); });
    }
  }
  run.run(PC_KW_FLAG, [&] { hipLaunchKernelGGL(k_kw_flag, dim3(B), dim3(KW_THREADS), 0, st, a); });
  if (counts) run.run(PC_KW_FLAG, [&] { hipLaunchKernelGGL(k_kw_tighten_count, dim3(B), dim3(KW_THREADS), 0, st, t); });
  return run.rc;
}


// ================================================================================================================
// Dual ascent on the subproblem LP of a batch of BaB domains (gnnb_k_dual.h; lp_producer.py LayerGraphLP.dual_ascent_host; stands in for
// the LP of reference plnn/conv_kwinter_gen.py:179-555 where only its optimum and a primal / dual point near it are needed)
// ================================================================================================================
extern "C" size_t gnnb_dual_workspace_bytes(const gnnb_t* h, int B) {
  if (!h || !h->bound || B < 1) return 0;
  return (size_t)B * dual_ws_doubles(h->R, h->N[0]) * sizeof(double);
}

extern "C" int gnnb_dual_ascent(gnnb_t* h, const gnnb_dual_batch* in, int B, int n_iter, double lr, double* alpha, double* beta, int warm,
                                double* bound, double* grad_alpha, double* grad_beta, float* const* dual, float* const* primal, float* x_lp,
                                float* lb32_prop, void* workspace, size_t workspace_bytes, void* stream) {
  size_t lds = 0;
  if (int rc = kw_preflight(h, "gnnb_dual_ascent", in ? &in->n_graph : nullptr, &lds)) return rc;
  if (!alpha || !beta || !bound || !workspace || B < 1 || n_iter < 0)
    return fail(GNNB_E_INVALID, "gnnb_dual_ascent: null argument, batch size %d < 1 or %d iterations", B, n_iter);
  if (!in->lb || !in->ub || !in->x_lo || !in->x_hi || !in->prop_w || !in->prop_b || !in->mask)
    return fail(GNNB_E_INVALID, "gnnb_dual_ascent: null input pointer");
  if ((grad_alpha == nullptr) != (grad_beta == nullptr)) return fail(GNNB_E_INVALID, "gnnb_dual_ascent: grad_alpha and grad_beta go together");
  if ((dual == nullptr) != (primal == nullptr) || (dual == nullptr) != (x_lp == nullptr))
    return fail(GNNB_E_INVALID, "gnnb_dual_ascent: dual, primal and x_lp go together");
  const size_t need = gnnb_dual_workspace_bytes(h, B);
  if (workspace_bytes < need) return fail(GNNB_E_NOMEM, "gnnb_dual_ascent: workspace %zu bytes, need %zu", workspace_bytes, need);
  DualArgs a{};
  a.net = h->kw_net;
  a.n_iter = n_iter; a.warm = warm ? 1 : 0; a.lr = lr;
  for (int k = 1; k <= a.net.L; ++k) {
    if (!in->lb[k - 1] || !in->ub[k - 1]) return fail(GNNB_E_INVALID, "gnnb_dual_ascent: null bounds pointer for graph layer %d", k);
    const int q = h->relu_q[k];
    if (dual && (!dual[k - 1] || !primal[q - 1] || !primal[q])) return fail(GNNB_E_INVALID, "gnnb_dual_ascent: null scorer array (layer %d)", k);
    a.lb[k] = in->lb[k - 1]; a.ub[k] = in->ub[k - 1];
    if (dual) { a.dual[k] = dual[k - 1]; a.z_pre[k] = primal[q - 1]; a.z_post[k] = primal[q]; }
  }
  if (dual) {
    if (!primal[h->n_fixed]) return fail(GNNB_E_INVALID, "gnnb_dual_ascent: null primals[-1]");
    a.z_out = primal[h->n_fixed];
  }
  a.x_lo = in->x_lo; a.x_hi = in->x_hi; a.prop_w = in->prop_w; a.prop_b = in->prop_b; a.mask = in->mask;
  a.alpha = alpha; a.beta = beta; a.bound = bound; a.grad_alpha = grad_alpha; a.grad_beta = grad_beta;
  a.x_lp = x_lp; a.lb32_prop = lb32_prop;
  a.ws = (double*)workspace; a.ws_stride = (long)dual_ws_doubles(a.net.R, a.net.N[0]);
  hipStream_t st = (hipStream_t)stream;
  Launcher run{h, st};
  run.run(PC_DUAL, [&] { hipLaunchKernelGGL(k_dual_ascent, dim3(B), dim3(DUAL_THREADS), lds, st, a); });
  return run.rc;
}


// ================================================================================================================
// A branch-and-bound frontier in device memory (gnnb_k_frontier.h): the steps of a round between the batch entry
// points above.  Each checks everything before its first launch and launches on the caller's stream.
// ================================================================================================================
static int frontier_preflight(const gnnb_t* h, const char* who, int K, const int* n_graph) {
  size_t lds = 0;
  if (K < 1 || K > 32767) return fail(GNNB_E_INVALID, "%s: K = %d outside 1..32767", who, K);
  return kw_preflight(h, who, n_graph, &lds);
}

static FrShape fr_shape(const gnnb_t* h) {
  FrShape s{};
  const KwNet& n = h->kw_net;
  s.L = n.L; s.R = n.R;
  for (int k = 0; k <= n.L; ++k) { s.N[k] = n.N[k]; s.off[k] = n.off[k]; }
  s.N[n.L + 1] = 1;                                     // the property node
  return s;
}

static int fr_pool(const gnnb_t* h, const char* who, const gnnb_pool* pool, FrPool* p) {
  if (!pool->mask || !pool->lb || !pool->ub || !pool->alpha || !pool->beta || !pool->bound || !pool->open || pool->capacity < 1)
    return fail(GNNB_E_INVALID, "%s: null pool array or capacity %d < 1", who, pool->capacity);
  p->mask = pool->mask; p->alpha = pool->alpha; p->beta = pool->beta; p->bound = pool->bound; p->open = pool->open; p->cap = pool->capacity;
  for (int k = 1; k <= h->kw_net.L + 1; ++k) {
    if (!pool->lb[k - 1] || !pool->ub[k - 1]) return fail(GNNB_E_INVALID, "%s: null pool bounds pointer for graph layer %d", who, k);
    p->lb[k] = pool->lb[k - 1]; p->ub[k] = pool->ub[k - 1];
  }
  return GNNB_OK;
}

// the pool of many jobs (section 7.4): the plan's segments fill it
static int fr_plan_pool(const gnnb_t* h, const char* who, const gnnb_plan* plan, const gnnb_pool* pool, FrPool* p) {
  if (int rc = fr_pool(h, who, pool, p)) return rc;
  if ((long)plan->segments * plan->seg_cap != pool->capacity)
    return fail(GNNB_E_INVALID, "%s: %d segments of %d slots in a pool of %d", who, plan->segments, plan->seg_cap, pool->capacity);
  return GNNB_OK;
}

extern "C" int gnnb_frontier_gather(gnnb_t* h, const gnnb_pool* pool, const int32_t* slots, int K, const double* x_lo, const double* x_hi,
                                    int8_t* mask, double* const* lb, double* const* ub, float* const* lb32, float* const* ub32, double* alpha,
                                    double* beta, float* scorer_mask, void* stream) {
  if (int rc = frontier_preflight(h, "gnnb_frontier_gather", K, pool ? &pool->n_graph : nullptr)) return rc;
  if (!slots || !x_lo || !x_hi || !mask || !lb || !ub || !lb32 || !ub32 || !alpha || !beta || !scorer_mask)
    return fail(GNNB_E_INVALID, "gnnb_frontier_gather: null argument");
  FrGatherArgs a{};
  a.s = fr_shape(h);
  if (int rc = fr_pool(h, "gnnb_frontier_gather", pool, &a.p)) return rc;
  for (int k = 0; k <= a.s.L + 1; ++k) {
    if (!lb32[k] || !ub32[k] || (k > 0 && (!lb[k - 1] || !ub[k - 1]))) return fail(GNNB_E_INVALID, "gnnb_frontier_gather: null output pointer for graph layer %d", k);
    a.lb32[k] = lb32[k]; a.ub32[k] = ub32[k];
    if (k > 0) { a.lb[k] = lb[k - 1]; a.ub[k] = ub[k - 1]; }
  }
  a.slots = slots; a.K = K; a.x_lo = x_lo; a.x_hi = x_hi; a.mask = mask; a.alpha = alpha; a.beta = beta; a.amb = scorer_mask;
  hipStream_t st = (hipStream_t)stream;
  Launcher run{h, st};
  run.run(PC_FR_GATHER, [&] { hipLaunchKernelGGL(k_frontier_gather, dim3(K, FR_SPLIT), dim3(FR_THREADS), 0, st, a); });
  return run.rc;
}

extern "C" int gnnb_frontier_expand(gnnb_t* h, const gnnb_pool* pool, const int32_t* slots, const int32_t* decisions, int K, int8_t* mask,
                                    double* const* parent_lb, double* const* parent_ub, int32_t* split_layer, double* alpha, double* beta,
                                    int32_t* live, void* stream) {
  if (int rc = frontier_preflight(h, "gnnb_frontier_expand", K, pool ? &pool->n_graph : nullptr)) return rc;
  if (!slots || !decisions || !mask || !parent_lb || !parent_ub || !split_layer || !alpha || !beta || !live)
    return fail(GNNB_E_INVALID, "gnnb_frontier_expand: null argument");
  FrExpandArgs a{};
  a.s = fr_shape(h);
  if (int rc = fr_pool(h, "gnnb_frontier_expand", pool, &a.p)) return rc;
  for (int k = 1; k <= a.s.L + 1; ++k) {
    if (!parent_lb[k - 1] || !parent_ub[k - 1]) return fail(GNNB_E_INVALID, "gnnb_frontier_expand: null output pointer for graph layer %d", k);
    a.ch.lb[k] = parent_lb[k - 1]; a.ch.ub[k] = parent_ub[k - 1];
  }
  a.slots = slots; a.decisions = decisions; a.K = K; a.ch.mask = mask; a.split = split_layer; a.ch.alpha = alpha; a.ch.beta = beta; a.live = live;
  hipStream_t st = (hipStream_t)stream;
  Launcher run{h, st};
  run.run(PC_FR_EXPAND, [&] { hipLaunchKernelGGL(k_frontier_expand, dim3(2 * K, FR_SPLIT), dim3(FR_THREADS), 0, st, a); });
  return run.rc;
}

// What the gnnb_net_* entry points check of the handle, after their own sizes: it exists, and its bound network passes kw_preflight.
static int net_preflight(const gnnb_t* h, const char* who) {
  if (!h) return fail(GNNB_E_INVALID, "%s: null handle", who);           // (before h->bound is read)
  const int ng = h->bound ? h->kw_net.L + 2 : 0;
  size_t lds = 0;
  return kw_preflight(h, who, &ng, &lds);
}

// The walk's argument block but for the caller's arrays: the network, where each layer's activations start, one point per workgroup,
// and the workspace at ws_stride doubles per workgroup.
static NetArgs net_args(const gnnb_t* h, void* workspace, long ws_stride) {
  NetArgs a{};
  a.net = h->kw_net; a.n_starts = 1;
  a.ws = (double*)workspace; a.ws_stride = ws_stride; a.width = net_eval_width(a.net);
  for (int k = 0; k <= a.net.L; ++k) a.act_off[k + 1] = a.act_off[k] + a.net.N[k];
  return a;
}

extern "C" size_t gnnb_net_eval_workspace_bytes(const gnnb_t* h, int B) {
  if (!h || !h->bound || B < 1) return 0;
  return (size_t)B * 2 * net_eval_width(h->kw_net) * sizeof(double);
}

extern "C" int gnnb_net_eval(gnnb_t* h, const float* x, const float* prop_w, const float* prop_b, int B, double* out, void* workspace,
                             size_t workspace_bytes, void* stream) {
  const char* who = "gnnb_net_eval";
  if (B < 1) return fail(GNNB_E_INVALID, "%s: B = %d", who, B);
  if (int rc = net_preflight(h, who)) return rc;
  if (!x || !prop_w || !prop_b || !out || !workspace) return fail(GNNB_E_INVALID, "%s: null argument", who);
  const size_t need = gnnb_net_eval_workspace_bytes(h, B);
  if (workspace_bytes < need) return fail(GNNB_E_NOMEM, "%s: workspace %zu bytes, need %zu", who, workspace_bytes, need);
  NetArgs a = net_args(h, workspace, 2L * net_eval_width(h->kw_net));
  a.x = x; a.prop_w = prop_w; a.prop_b = prop_b; a.val = out;
  hipStream_t st = (hipStream_t)stream;
  Launcher run{h, st};
  run.run(PC_NET_EVAL, [&] { hipLaunchKernelGGL(k_net_eval, dim3(B), dim3(NET_THREADS), 0, st, a); });
  return run.rc;
}

// ---- projected signed-gradient descent from a batch of points (reference plnn/conv_kwinter_gen.py:54-135) ----
extern "C" size_t gnnb_net_descend_workspace_bytes(const gnnb_t* h, int B) {
  if (!h || !h->bound || B < 1) return 0;
  return (size_t)B * net_descend_doubles(h->kw_net) * sizeof(double);
}

extern "C" int gnnb_net_descend(gnnb_t* h, const float* x0, const double* x_lo, const double* x_hi, const float* prop_w, const float* prop_b, int B,
                                int n_steps, double step, float* x_best, double* value, double* grad0, int32_t* steps_taken, void* workspace,
                                size_t workspace_bytes, void* stream) {
  const char* who = "gnnb_net_descend";
  if (B < 1) return fail(GNNB_E_INVALID, "%s: B = %d", who, B);
  if (n_steps < 0) return fail(GNNB_E_INVALID, "%s: n_steps = %d", who, n_steps);
  if (!(step > 0.0 && step <= 1.0)) return fail(GNNB_E_INVALID, "%s: step = %g (0 < . <= 1)", who, step);
  if (int rc = net_preflight(h, who)) return rc;
  if (!x0 || !x_lo || !x_hi || !prop_w || !prop_b || !x_best || !value || !workspace) return fail(GNNB_E_INVALID, "%s: null argument", who);
  if (x_best == x0) return fail(GNNB_E_INVALID, "%s: x_best must not overlap x0", who);
  const size_t need = gnnb_net_descend_workspace_bytes(h, B);
  if (workspace_bytes < need) return fail(GNNB_E_NOMEM, "%s: workspace %zu bytes, need %zu", who, workspace_bytes, need);
  NetArgs a = net_args(h, workspace, net_descend_doubles(h->kw_net));
  a.x = x0; a.x_lo = x_lo; a.x_hi = x_hi; a.prop_w = prop_w; a.prop_b = prop_b;
  a.n_steps = n_steps; a.step = step;
  a.xb = x_best; a.val = value; a.grad0 = grad0; a.steps_taken = steps_taken;
  hipStream_t st = (hipStream_t)stream;
  Launcher run{h, st};
  run.run(PC_NET_DESCEND, [&] { hipLaunchKernelGGL(k_net_descend, dim3(B), dim3(NET_THREADS), 0, st, a); });
  return run.rc;
}

// ---- the upper bound from many starts (reference plnn/conv_kwinter_gen.py:20-52 and :54-135) ----
extern "C" int gnnb_net_starts(gnnb_t* h, const float* x0, const double* x_lo, const double* x_hi, int B, int R, uint64_t seed, float* starts,
                               void* stream) {
  const char* who = "gnnb_net_starts";
  if (B < 1) return fail(GNNB_E_INVALID, "%s: B = %d", who, B);
  if (R < 0 || R > NS_MAX_RANDOM) return fail(GNNB_E_INVALID, "%s: R = %d outside 0..%d", who, R, NS_MAX_RANDOM);
  if (int rc = net_preflight(h, who)) return rc;
  if (!x0 || !x_lo || !x_hi || !starts) return fail(GNNB_E_INVALID, "%s: null argument", who);
  if (starts == x0) return fail(GNNB_E_INVALID, "%s: starts must not overlap x0", who);
  NetStartsArgs a{};
  a.x0 = x0; a.x_lo = x_lo; a.x_hi = x_hi; a.starts = starts; a.N0 = h->kw_net.N[0]; a.R = R; a.seed = seed;
  hipStream_t st = (hipStream_t)stream;
  Launcher run{h, st};
  run.run(PC_NET_STARTS, [&] { hipLaunchKernelGGL(k_net_starts, dim3(B, (R + NS_SLOTS) / NS_SLOTS), dim3(FR_THREADS), 0, st, a); });
  return run.rc;
}

extern "C" int gnnb_net_descend_starts_tile(void) { return NS_TILE; }

struct NsWs { size_t val, xb, total; };              // byte offsets in gnnb_net_descend_starts' workspace: the tiles' activations and gradients at 0
static NsWs ns_ws_layout(const gnnb_t* h, int B, int n_starts) {
  const size_t tiles = (size_t)B * ((n_starts + NS_TILE - 1) / NS_TILE);
  NsWs w;
  w.val = (tiles * NS_TILE * net_descend_doubles(h->kw_net) * sizeof(double) + 255) & ~(size_t)255;
  w.xb = w.val + (((size_t)B * n_starts * sizeof(double) + 255) & ~(size_t)255);
  w.total = w.xb + (((size_t)B * n_starts * h->kw_net.N[0] * sizeof(float) + 255) & ~(size_t)255);
  return w;
}

extern "C" size_t gnnb_net_descend_starts_workspace_bytes(const gnnb_t* h, int B, int n_starts) {
  if (!h || !h->bound || B < 1 || n_starts < 1 || n_starts > NS_MAX_RANDOM + 1) return 0;
  return ns_ws_layout(h, B, n_starts).total;
}

extern "C" int gnnb_net_descend_starts(gnnb_t* h, const float* starts, int n_starts, const double* x_lo, const double* x_hi, const float* prop_w,
                                       const float* prop_b, int B, int n_steps, double step, float* x_best, double* value, int32_t* start_index,
                                       double* start_value, int32_t* start_steps, void* workspace, size_t workspace_bytes, void* stream) {
  const char* who = "gnnb_net_descend_starts";
  if (B < 1) return fail(GNNB_E_INVALID, "%s: B = %d", who, B);
  if (n_starts < 1 || n_starts > NS_MAX_RANDOM + 1) return fail(GNNB_E_INVALID, "%s: n_starts = %d outside 1..%d", who, n_starts, NS_MAX_RANDOM + 1);
  if (n_steps < 0) return fail(GNNB_E_INVALID, "%s: n_steps = %d", who, n_steps);
  if (!(step > 0.0 && step <= 1.0)) return fail(GNNB_E_INVALID, "%s: step = %g (0 < . <= 1)", who, step);
  if (int rc = net_preflight(h, who)) return rc;
  if (!starts || !x_lo || !x_hi || !prop_w || !prop_b || !x_best || !value || !workspace) return fail(GNNB_E_INVALID, "%s: null argument", who);
  if (x_best == starts) return fail(GNNB_E_INVALID, "%s: x_best must not overlap starts", who);
  if ((long)B * ((n_starts + NS_TILE - 1) / NS_TILE) > 0x7fffffffL) return fail(GNNB_E_INVALID, "%s: B = %d rows of %d starts: too many tiles", who, B, n_starts);
  const NsWs w = ns_ws_layout(h, B, n_starts);
  if (workspace_bytes < w.total) return fail(GNNB_E_NOMEM, "%s: workspace %zu bytes, need %zu", who, workspace_bytes, w.total);
  const int tiles = B * ((n_starts + NS_TILE - 1) / NS_TILE);
  NetArgs a = net_args(h, workspace, (long)NS_TILE * net_descend_doubles(h->kw_net));
  a.x = starts; a.n_starts = n_starts; a.x_lo = x_lo; a.x_hi = x_hi; a.prop_w = prop_w; a.prop_b = prop_b;
  a.n_steps = n_steps; a.step = step;
  a.val = (double*)((char*)workspace + w.val); a.xb = (float*)((char*)workspace + w.xb); a.steps_taken = start_steps;
  NetPickArgs p{};
  p.xb = a.xb; p.val = a.val; p.n_starts = n_starts; p.N0 = a.net.N[0];
  p.x_best = x_best; p.value = value; p.start_index = start_index; p.start_value = start_value;
  hipStream_t st = (hipStream_t)stream;
  Launcher run{h, st};
  run.run(PC_NET_DESCEND_TILE, [&] { hipLaunchKernelGGL(k_net_descend_tile<NS_TILE>, dim3(tiles), dim3(NET_THREADS), 0, st, a); });
  run.run(PC_NET_STARTS_PICK, [&] { hipLaunchKernelGGL(k_net_starts_pick, dim3(B), dim3(FR_THREADS), 0, st, p); });
  return run.rc;
}

struct FrWs { size_t undecided, dest, total; };     // byte offsets in gnnb_frontier_commit's workspace: the resolved masks at 0
static FrWs fr_ws_layout(const gnnb_t* h, int rows) {       // rows: the child rows of the commit (2K; K << depth in a round of section 7.20)
  FrWs w;
  w.undecided = ((size_t)rows * h->R + 255) & ~(size_t)255;
  w.dest = w.undecided + (((size_t)rows * sizeof(int32_t) + 255) & ~(size_t)255);
  w.total = w.dest + (((size_t)rows * sizeof(int32_t) + 255) & ~(size_t)255);
  return w;
}

extern "C" size_t gnnb_frontier_commit_workspace_bytes(const gnnb_t* h, int K) {
  if (!h || !h->bound || K < 1) return 0;
  return fr_ws_layout(h, 2 * K).total;
}

// A gnnb_children / gnnb_children_rw checked against the pool's n_graph, as the kernels' struct of it (lb / ub of graph layer k at [k]).
template <class Ch, class Rows>
static int fr_children(const gnnb_t* h, const char* who, const Ch* ch, int n_graph, Rows* r) {
  if (ch->n_graph != n_graph) return fail(GNNB_E_INVALID, "%s: the children have %d graph layers, the pool %d", who, ch->n_graph, n_graph);
  if (!ch->mask || !ch->lb || !ch->ub || !ch->infeasible || !ch->bound || !ch->alpha || !ch->beta || !ch->ub_value || !ch->live)
    return fail(GNNB_E_INVALID, "%s: null array among the children's", who);
  for (int k = 1; k <= h->kw_net.L + 1; ++k) {
    if (!ch->lb[k - 1] || !ch->ub[k - 1]) return fail(GNNB_E_INVALID, "%s: null bounds pointer for graph layer %d", who, k);
    r->lb[k] = ch->lb[k - 1]; r->ub[k] = ch->ub[k - 1];
  }
  r->mask = ch->mask; r->alpha = ch->alpha; r->beta = ch->beta;
  r->infeasible = ch->infeasible; r->bound = ch->bound; r->ubv = ch->ub_value; r->live = ch->live;
  return GNNB_OK;
}

// What gnnb_frontier_commit, gnnb_frontier_commit_jobs and gnnb_frontier_commit_depth share once their own preflight is through: the
// `rows` children (2n; n << depth) of the parents in slots[0..n), checked, then resolve, decide (the caller's launch: one workgroup on the
// pool, or one per plan entry) and store.  plan: null, or the plan whose segments the pool must hold.
template <class Decide>
static int fr_commit(gnnb_t* h, const char* who, const gnnb_pool* pool, const gnnb_plan* plan, const int32_t* slots, int n, int rows,
                     const gnnb_children* ch, double eps, double* state, void* workspace, size_t workspace_bytes, void* stream, Decide decide) {
  FrCommitArgs a{};
  if (int rc = fr_children(h, who, ch, pool->n_graph, &a.ch)) return rc;
  if (!(eps >= 0.0)) return fail(GNNB_E_INVALID, "%s: eps = %g", who, eps);
  const FrWs ws = fr_ws_layout(h, rows);
  if (workspace_bytes < ws.total) return fail(GNNB_E_NOMEM, "%s: workspace %zu bytes, need %zu", who, workspace_bytes, ws.total);
  a.s = fr_shape(h);
  if (int rc = plan ? fr_plan_pool(h, who, plan, pool, &a.p) : fr_pool(h, who, pool, &a.p)) return rc;
  a.slots = slots; a.K = n; a.eps = eps; a.state = state;
  a.rmask = (int8_t*)workspace;
  a.undecided = (int32_t*)((char*)workspace + ws.undecided);
  a.dest = (int32_t*)((char*)workspace + ws.dest);
  hipStream_t st = (hipStream_t)stream;
  Launcher run{h, st};
  run.run(PC_FR_RESOLVE, [&] { hipLaunchKernelGGL(k_frontier_resolve, dim3(rows), dim3(FR_THREADS), 0, st, a); });
  decide(run, st, a);
  run.run(PC_FR_STORE, [&] { hipLaunchKernelGGL(k_frontier_store, dim3(rows, FR_SPLIT), dim3(FR_THREADS), 0, st, a); });
  return run.rc;
}

extern "C" int gnnb_frontier_commit(gnnb_t* h, const gnnb_pool* pool, const int32_t* slots, int K, const gnnb_children* ch, double eps,
                                    double decision_bound, double* state, void* workspace, size_t workspace_bytes, void* stream) {
  const char* who = "gnnb_frontier_commit";
  if (int rc = frontier_preflight(h, who, K, pool ? &pool->n_graph : nullptr)) return rc;
  if (!slots || !ch || !state || !workspace) return fail(GNNB_E_INVALID, "%s: null argument", who);
  return fr_commit(h, who, pool, nullptr, slots, K, 2 * K, ch, eps, state, workspace, workspace_bytes, stream,
                   [&](Launcher& run, hipStream_t st, FrCommitArgs& a) {
                     a.decision_bound = decision_bound;
                     run.run(PC_FR_DECIDE, [&] { hipLaunchKernelGGL(k_frontier_decide, dim3(1), dim3(FR_THREADS), 0, st, a); });
                   });
}

// ---- several ReLUs per parent while a round is underfilled: C = 2^depth children per parent ----
static int fr_depth_preflight(const gnnb_t* h, const char* who, int K, int depth, const int* n_graph) {
  if (depth < 1 || depth > FR_MAX_DEPTH) return fail(GNNB_E_INVALID, "%s: depth = %d outside 1..%d", who, depth, FR_MAX_DEPTH);
  if (K >= 1 && ((long)K << depth) > 65534)           // (the sizes first: they need no handle.  K < 1: frontier_preflight's)
    return fail(GNNB_E_INVALID, "%s: K = %d parents at depth %d are %ld child rows, above 65534", who, K, depth, (long)K << depth);
  return frontier_preflight(h, who, K, n_graph);
}

extern "C" int gnnb_frontier_expand_depth(gnnb_t* h, const gnnb_pool* pool, const int32_t* slots, int K, int depth, const int32_t* cand0,
                                          const int32_t* cand_dec, int8_t* mask, double* const* parent_lb, double* const* parent_ub,
                                          int32_t* split_layer, double* alpha, double* beta, int32_t* live, void* stream) {
  const char* who = "gnnb_frontier_expand_depth";
  if (int rc = fr_depth_preflight(h, who, K, depth, pool ? &pool->n_graph : nullptr)) return rc;
  if (!slots || !cand0 || !cand_dec || !mask || !parent_lb || !parent_ub || !split_layer || !alpha || !beta || !live)
    return fail(GNNB_E_INVALID, "%s: null argument", who);
  FrExpandDepthArgs a{};
  a.s = fr_shape(h);
  if (int rc = fr_pool(h, who, pool, &a.p)) return rc;
  for (int k = 1; k <= a.s.L + 1; ++k) {
    if (!parent_lb[k - 1] || !parent_ub[k - 1]) return fail(GNNB_E_INVALID, "%s: null output pointer for graph layer %d", who, k);
    a.ch.lb[k] = parent_lb[k - 1]; a.ch.ub[k] = parent_ub[k - 1];
  }
  a.slots = slots; a.cand0 = cand0; a.cand_dec = cand_dec; a.K = K; a.depth = depth;
  a.ch.mask = mask; a.split = split_layer; a.ch.alpha = alpha; a.ch.beta = beta; a.live = live;
  hipStream_t st = (hipStream_t)stream;
  Launcher run{h, st};
  run.run(PC_FR_EXPAND, [&] { hipLaunchKernelGGL(k_frontier_expand_depth, dim3(K << depth, FR_SPLIT), dim3(FR_THREADS), 0, st, a); });
  return run.rc;
}

extern "C" size_t gnnb_frontier_commit_depth_workspace_bytes(const gnnb_t* h, int K, int depth) {
  if (!h || !h->bound || K < 1 || depth < 1 || depth > FR_MAX_DEPTH || ((long)K << depth) > 65534) return 0;
  return fr_ws_layout(h, K << depth).total;
}

extern "C" int gnnb_frontier_commit_depth(gnnb_t* h, const gnnb_pool* pool, const int32_t* slots, int K, int depth, const gnnb_children* ch,
                                          double eps, double decision_bound, double* state, void* workspace, size_t workspace_bytes,
                                          void* stream) {
  const char* who = "gnnb_frontier_commit_depth";
  if (int rc = fr_depth_preflight(h, who, K, depth, pool ? &pool->n_graph : nullptr)) return rc;
  if (!slots || !ch || !state || !workspace) return fail(GNNB_E_INVALID, "%s: null argument", who);
  return fr_commit(h, who, pool, nullptr, slots, K, K << depth, ch, eps, state, workspace, workspace_bytes, stream,
                   [&](Launcher& run, hipStream_t st, FrCommitArgs& a) {
                     a.decision_bound = decision_bound;
                     run.run(PC_FR_DECIDE, [&] { hipLaunchKernelGGL(k_frontier_decide_depth, dim3(1), dim3(FR_THREADS), 0, st, a, depth); });
                   });
}

// ---- many jobs in one pool: a pool of plan->segments segments of plan->seg_cap slots, one record per segment ----
// Everything a kernel would trust is checked here on the host copy of the plan: the entries tile the rows [0, n) in order.
static int fr_plan(const gnnb_t* h, const char* who, const gnnb_plan* plan, const int* n_graph, FrPlan* j) {
  if (!plan) return fail(GNNB_E_INVALID, "%s: null plan", who);
  if (plan->n_entries < 1 || plan->n < 1 || plan->n > 32767)
    return fail(GNNB_E_INVALID, "%s: %d plan entries, n = %d rows (at least one entry, n in 1..32767)", who, plan->n_entries, plan->n);
  size_t lds = 0;
  if (int rc = kw_preflight(h, who, n_graph, &lds)) return rc;
  if (!plan->host || !plan->device) return fail(GNNB_E_INVALID, "%s: null plan array", who);
  if (plan->segments < 1 || plan->seg_cap < 1 || (long)plan->segments * plan->seg_cap > 2147483647L)
    return fail(GNNB_E_INVALID, "%s: %d segments of %d slots", who, plan->segments, plan->seg_cap);
  long row = 0;
  for (int e = 0; e < plan->n_entries; ++e) {
    const int seg = plan->host[3 * e], row0 = plan->host[3 * e + 1], k = plan->host[3 * e + 2];
    if (seg < 0 || seg >= plan->segments) return fail(GNNB_E_INVALID, "%s: plan entry %d names segment %d outside the pool's 0..%d", who, e, seg, plan->segments - 1);
    if (k < 1) return fail(GNNB_E_INVALID, "%s: plan entry %d has k = %d < 1", who, e, k);
    if (row0 != row) return fail(GNNB_E_INVALID, "%s: plan entry %d starts at row %d, the entries before it end at %ld", who, e, row0, row);
    row += k;
    if (row > plan->n) break;
  }
  if (row != plan->n) return fail(GNNB_E_INVALID, "%s: the plan's entries hold %ld rows, n = %d", who, row, plan->n);
  j->plan = plan->device; j->n_entries = plan->n_entries; j->n = plan->n; j->S = plan->segments; j->seg_cap = plan->seg_cap;
  return GNNB_OK;
}

extern "C" int gnnb_frontier_pick_jobs(gnnb_t* h, const gnnb_pool* pool, const gnnb_plan* plan, const double* state, int32_t* slots,
                                       int32_t* row_seg, void* stream) {
  FrPickArgs a{};
  if (int rc = fr_plan(h, "gnnb_frontier_pick_jobs", plan, pool ? &pool->n_graph : nullptr, &a.j)) return rc;
  if (!state || !slots || !row_seg) return fail(GNNB_E_INVALID, "gnnb_frontier_pick_jobs: null argument");
  if (int rc = fr_plan_pool(h, "gnnb_frontier_pick_jobs", plan, pool, &a.p)) return rc;
  a.state = state; a.slots = slots; a.row_seg = row_seg;
  hipStream_t st = (hipStream_t)stream;
  Launcher run{h, st};
  run.run(PC_FR_PICK_JOBS, [&] { hipLaunchKernelGGL(k_frontier_pick_jobs, dim3(a.j.n_entries), dim3(FR_THREADS), 0, st, a); });
  return run.rc;
}

extern "C" int gnnb_frontier_rows_jobs(gnnb_t* h, const gnnb_plan* plan, const int32_t* row_seg, const double* seg_x_lo, const double* seg_x_hi,
                                       const float* seg_prop_w, const float* seg_prop_b, double* x_lo, double* x_hi, float* prop_w, float* prop_b,
                                       double* child_x_lo, double* child_x_hi, float* child_prop_w, float* child_prop_b, void* stream) {
  FrRowsArgs a{};
  const int ng = (h && h->bound) ? h->kw_net.L + 2 : 0;
  if (int rc = fr_plan(h, "gnnb_frontier_rows_jobs", plan, &ng, &a.j)) return rc;
  if (!row_seg || !seg_x_lo || !seg_x_hi || !seg_prop_w || !seg_prop_b || !x_lo || !x_hi || !prop_w || !prop_b || !child_x_lo || !child_x_hi ||
      !child_prop_w || !child_prop_b)
    return fail(GNNB_E_INVALID, "gnnb_frontier_rows_jobs: null argument");
  a.N0 = h->kw_net.N[0]; a.NL = h->kw_net.N[h->kw_net.L];
  a.row_seg = row_seg; a.seg_x_lo = seg_x_lo; a.seg_x_hi = seg_x_hi; a.seg_pw = seg_prop_w; a.seg_pb = seg_prop_b;
  a.x_lo[0] = x_lo; a.x_hi[0] = x_hi; a.pw[0] = prop_w; a.pb[0] = prop_b;
  a.x_lo[1] = child_x_lo; a.x_hi[1] = child_x_hi; a.pw[1] = child_prop_w; a.pb[1] = child_prop_b;
  hipStream_t st = (hipStream_t)stream;
  Launcher run{h, st};
  run.run(PC_FR_ROWS_JOBS, [&] { hipLaunchKernelGGL(k_frontier_rows_jobs, dim3(3 * a.j.n, FR_SPLIT), dim3(FR_THREADS), 0, st, a); });
  return run.rc;
}

extern "C" size_t gnnb_frontier_commit_jobs_workspace_bytes(const gnnb_t* h, int n) {
  if (!h || !h->bound || n < 1) return 0;
  return fr_ws_layout(h, 2 * n).total;
}

extern "C" int gnnb_frontier_commit_jobs(gnnb_t* h, const gnnb_pool* pool, const gnnb_plan* plan, const int32_t* slots, const gnnb_children* ch,
                                         double eps, const double* decision_bound, double* state, void* workspace, size_t workspace_bytes,
                                         void* stream) {
  const char* who = "gnnb_frontier_commit_jobs";
  FrPlan j{};
  if (int rc = fr_plan(h, who, plan, pool ? &pool->n_graph : nullptr, &j)) return rc;
  if (!slots || !ch || !decision_bound || !state || !workspace) return fail(GNNB_E_INVALID, "%s: null argument", who);
  return fr_commit(h, who, pool, plan, slots, j.n, 2 * j.n, ch, eps, state, workspace, workspace_bytes, stream,
                   [&](Launcher& run, hipStream_t st, FrCommitArgs& a) {
                     run.run(PC_FR_DECIDE_JOBS, [&] { hipLaunchKernelGGL(k_frontier_decide_jobs, dim3(j.n_entries), dim3(FR_THREADS), 0, st, a, j, decision_bound); });
                   });
}

// ---- the BaBSR fall-back below a branching threshold (reference plnn/relu_conv_gnnkwthreshold.py:151-195, the
// decision rule of plnn/kw_score_conv.py:115-156) ----
extern "C" size_t gnnb_frontier_fallback_workspace_bytes(const gnnb_t* h, int K) {
  if (!h || !h->bound || K < 1) return 0;
  return (size_t)K * FC_COUNT * sizeof(int32_t);
}

// The checks gnnb_frontier_fallback and gnnb_frontier_fallback_jobs share on a gnnb_fallback, and its values as the kernels' arguments.
static int fr_fallback_in(const char* who, const gnnb_fallback* in, FrFallbackArgs* a) {
  if (!in->live || !in->infeasible || !in->bound || !in->scores || !in->intercepts || !in->scorer_mask || !in->icp || !in->ineff ||
      (in->n_order > 0 && !in->random_order))
    return fail(GNNB_E_INVALID, "%s: null array among the inputs", who);
  if (!(in->branching_threshold > 0.0 && in->branching_threshold <= 1.0) || in->kwbd_threshold < 0 || in->decision_threshold != in->decision_threshold)
    return fail(GNNB_E_INVALID, "%s: branching_threshold = %g (0 < . <= 1), kwbd_threshold = %d (>= 0), decision_threshold = %g", who,
                in->branching_threshold, in->kwbd_threshold, in->decision_threshold);
  if (in->n_order < 0 || in->n_order > MAXL) return fail(GNNB_E_INVALID, "%s: random_order of %d layers (0..%d)", who, in->n_order, MAXL);
  a->live = in->live; a->infeasible = in->infeasible; a->bound = in->bound;
  a->scores = in->scores; a->icp_tb = in->intercepts; a->amb = in->scorer_mask;
  a->branching_threshold = in->branching_threshold; a->decision_threshold = in->decision_threshold;
  a->kwbd_threshold = in->kwbd_threshold; a->sparsest_layer = in->sparsest_layer; a->n_order = in->n_order;
  for (int q = 0; q < in->n_order; ++q) a->order[q] = in->random_order[q];
  a->icp = in->icp; a->ineff = in->ineff; a->pair_a = 1;
  return GNNB_OK;
}

extern "C" int gnnb_frontier_fallback(gnnb_t* h, const gnnb_pool* pool, const int32_t* slots, int K, const gnnb_fallback* in,
                                      double* gnn_improvement, int32_t* kw_decisions, int32_t* sel_rows, int32_t* sel_slots,
                                      int32_t* sel_decisions, int32_t* m, void* workspace, size_t workspace_bytes, void* stream) {
  const char* who = "gnnb_frontier_fallback";
  if (int rc = frontier_preflight(h, who, K, pool ? &pool->n_graph : nullptr)) return rc;
  if (!slots || !in || !gnn_improvement || !kw_decisions || !sel_rows || !sel_slots || !sel_decisions || !m || !workspace)
    return fail(GNNB_E_INVALID, "%s: null argument", who);
  FrFallbackArgs a{};
  if (int rc = fr_fallback_in(who, in, &a)) return rc;
  const size_t need = gnnb_frontier_fallback_workspace_bytes(h, K);
  if (workspace_bytes < need) return fail(GNNB_E_NOMEM, "%s: workspace %zu bytes, need %zu", who, workspace_bytes, need);
  a.s = fr_shape(h);
  if (int rc = fr_pool(h, who, pool, &a.p)) return rc;
  a.slots = slots; a.K = K;
  a.gnn_imp = gnn_improvement; a.kw_dec = kw_decisions; a.sel_rows = sel_rows; a.sel_slots = sel_slots; a.sel_dec = sel_decisions; a.m = m;
  a.cand = (int32_t*)workspace;
  hipStream_t st = (hipStream_t)stream;
  Launcher run{h, st};
  run.run(PC_FR_CANDIDATES, [&] { hipLaunchKernelGGL(k_frontier_candidates, dim3(K), dim3(FR_THREADS), 0, st, a); });
  run.run(PC_FR_FALLBACK, [&] { hipLaunchKernelGGL(k_frontier_fallback, dim3(1), dim3(64), 0, st, a); });
  return run.rc;
}

extern "C" int gnnb_frontier_choose(gnnb_t* h, const gnnb_pool* pool, int K, int m, const int32_t* sel_rows, const int32_t* sel_slots,
                                    const int32_t* sel_decisions, const int32_t* gnn_decisions, const double* gnn_improvement,
                                    const gnnb_children_rw* pa, const gnnb_children* pb, int32_t* ineff, double* kw_improvement,
                                    int32_t* used_kw, int32_t* decisions, void* stream) {
  const char* who = "gnnb_frontier_choose";
  if (int rc = frontier_preflight(h, who, K, pool ? &pool->n_graph : nullptr)) return rc;
  if (m < 0 || m > K) return fail(GNNB_E_INVALID, "%s: m = %d selected parents of K = %d", who, m, K);
  if (!sel_rows || !sel_slots || !sel_decisions || !gnn_decisions || !gnn_improvement || !pa || !ineff || !kw_improvement || !used_kw || !decisions ||
      (m > 0 && !pb))
    return fail(GNNB_E_INVALID, "%s: null argument", who);
  FrChooseArgs a{};
  a.s = fr_shape(h);
  if (int rc = fr_pool(h, who, pool, &a.p)) return rc;
  if (m > 0) {
    if (int rc = fr_children(h, who, pa, pool->n_graph, &a.A)) return rc;
    if (int rc = fr_children(h, who, pb, pool->n_graph, &a.B)) return rc;
  }
  a.K = K; a.m = m; a.sel_rows = sel_rows; a.sel_slots = sel_slots; a.sel_dec = sel_decisions; a.gnn_dec = gnn_decisions; a.gnn_imp = gnn_improvement;
  a.ineff = ineff; a.kw_imp = kw_improvement; a.used = used_kw; a.dec = decisions;
  hipStream_t st = (hipStream_t)stream;
  Launcher run{h, st};
  run.run(PC_FR_CHOOSE, [&] { hipLaunchKernelGGL(k_frontier_choose, dim3(1), dim3(FR_THREADS), 0, st, a); });
  if (m > 0) run.run(PC_FR_CHOOSE_COPY, [&] { hipLaunchKernelGGL(k_frontier_choose_copy, dim3(2 * m, FR_SPLIT), dim3(FR_THREADS), 0, st, a); });
  return run.rc;
}

// ---- the fall-back for many jobs in one pool: the two steps above per plan entry, on the segment's counter
// icp[segment] and table ineff[segment]; the selected parents of all entries form one dense list in plan order ----
struct FrFbWs { size_t st_rows, st_slots, st_dec, m_stage, total; };     // byte offsets in gnnb_frontier_fallback_jobs' workspace: the candidates at 0
static FrFbWs fr_fb_ws_layout(int n) {
  const auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
  FrFbWs w;
  w.st_rows = up((size_t)n * FC_COUNT * sizeof(int32_t));
  w.st_slots = w.st_rows + up((size_t)n * sizeof(int32_t));
  w.st_dec = w.st_slots + up((size_t)n * sizeof(int32_t));
  w.m_stage = w.st_dec + up((size_t)2 * n * sizeof(int32_t));
  w.total = w.m_stage + up((size_t)n * sizeof(int32_t));                 // (an entry holds at least one row: n_entries <= n)
  return w;
}

extern "C" size_t gnnb_frontier_fallback_jobs_workspace_bytes(const gnnb_t* h, int n) {
  if (!h || !h->bound || n < 1) return 0;
  return fr_fb_ws_layout(n).total;
}

extern "C" int gnnb_frontier_fallback_jobs(gnnb_t* h, const gnnb_pool* pool, const gnnb_plan* plan, const int32_t* slots, const gnnb_fallback* in,
                                           const double* seg_x_lo, const double* seg_x_hi, const float* seg_prop_w, const float* seg_prop_b,
                                           double* gnn_improvement, int32_t* kw_decisions, int32_t* sel_rows, int32_t* sel_slots,
                                           int32_t* sel_decisions, int32_t* m_entry, double* b_x_lo, double* b_x_hi, float* b_prop_w,
                                           float* b_prop_b, void* workspace, size_t workspace_bytes, void* stream) {
  const char* who = "gnnb_frontier_fallback_jobs";
  FrSelArgs sel{};
  if (int rc = fr_plan(h, who, plan, pool ? &pool->n_graph : nullptr, &sel.j)) return rc;
  if (!slots || !in || !seg_x_lo || !seg_x_hi || !seg_prop_w || !seg_prop_b || !gnn_improvement || !kw_decisions || !sel_rows || !sel_slots ||
      !sel_decisions || !m_entry || !b_x_lo || !b_x_hi || !b_prop_w || !b_prop_b || !workspace)
    return fail(GNNB_E_INVALID, "%s: null argument", who);
  FrFallbackArgs a{};
  if (int rc = fr_fallback_in(who, in, &a)) return rc;
  const int n = sel.j.n;
  const FrFbWs ws = fr_fb_ws_layout(n);
  if (workspace_bytes < ws.total) return fail(GNNB_E_NOMEM, "%s: workspace %zu bytes, need %zu", who, workspace_bytes, ws.total);
  a.s = fr_shape(h);
  if (int rc = fr_plan_pool(h, who, plan, pool, &a.p)) return rc;
  char* w = (char*)workspace;
  int32_t* m_stage = (int32_t*)(w + ws.m_stage);
  a.slots = slots; a.K = n;
  a.gnn_imp = gnn_improvement; a.kw_dec = kw_decisions;
  a.sel_rows = (int32_t*)(w + ws.st_rows); a.sel_slots = (int32_t*)(w + ws.st_slots); a.sel_dec = (int32_t*)(w + ws.st_dec); a.m = nullptr;
  a.cand = (int32_t*)w;
  sel.m_stage = m_stage; sel.st_rows = a.sel_rows; sel.st_slots = a.sel_slots; sel.st_dec = a.sel_dec;
  sel.sel_rows = sel_rows; sel.sel_slots = sel_slots; sel.sel_dec = sel_decisions; sel.m_entry = m_entry;
  sel.N0 = h->kw_net.N[0]; sel.NL = h->kw_net.N[h->kw_net.L];
  sel.seg_x_lo = seg_x_lo; sel.seg_x_hi = seg_x_hi; sel.seg_pw = seg_prop_w; sel.seg_pb = seg_prop_b;
  sel.b_x_lo = b_x_lo; sel.b_x_hi = b_x_hi; sel.b_pw = b_prop_w; sel.b_pb = b_prop_b;
  const FrPlan j = sel.j;
  hipStream_t st = (hipStream_t)stream;
  Launcher run{h, st};
  run.run(PC_FR_CANDIDATES, [&] { hipLaunchKernelGGL(k_frontier_candidates, dim3(n), dim3(FR_THREADS), 0, st, a); });
  run.run(PC_FR_FALLBACK_JOBS, [&] { hipLaunchKernelGGL(k_frontier_fallback_jobs, dim3(j.n_entries), dim3(64), 0, st, a, j, m_stage); });
  run.run(PC_FR_SELECT_JOBS, [&] { hipLaunchKernelGGL(k_frontier_select_jobs, dim3(1), dim3(FR_THREADS), 0, st, sel); });
  run.run(PC_FR_ROWS_SEL, [&] { hipLaunchKernelGGL(k_frontier_rows_sel, dim3(2 * n, FR_SPLIT), dim3(FR_THREADS), 0, st, sel); });
  return run.rc;
}

extern "C" int gnnb_frontier_choose_jobs(gnnb_t* h, const gnnb_pool* pool, const gnnb_plan* plan, int M, const int32_t* m_entry,
                                         const int32_t* sel_rows, const int32_t* sel_slots, const int32_t* sel_decisions,
                                         const int32_t* gnn_decisions, const double* gnn_improvement, const gnnb_children_rw* pa,
                                         const gnnb_children* pb, int32_t* ineff, double* kw_improvement, int32_t* used_kw, int32_t* decisions,
                                         void* stream) {
  const char* who = "gnnb_frontier_choose_jobs";
  FrPlan j{};
  if (plan && plan->n >= 1 && plan->n <= 32767 && (M < 0 || M > plan->n))      // (as K's range: before the handle is looked at)
    return fail(GNNB_E_INVALID, "%s: M = %d selected parents of n = %d", who, M, plan->n);
  if (int rc = fr_plan(h, who, plan, pool ? &pool->n_graph : nullptr, &j)) return rc;
  if (M < 0 || M > j.n) return fail(GNNB_E_INVALID, "%s: M = %d selected parents of n = %d", who, M, j.n);
  if (!m_entry || !sel_rows || !sel_slots || !sel_decisions || !gnn_decisions || !gnn_improvement || !pa || !ineff || !kw_improvement || !used_kw ||
      !decisions || (M > 0 && !pb))
    return fail(GNNB_E_INVALID, "%s: null argument", who);
  FrChooseArgs a{};
  a.s = fr_shape(h);
  if (int rc = fr_plan_pool(h, who, plan, pool, &a.p)) return rc;
  if (M > 0) {
    if (int rc = fr_children(h, who, pa, pool->n_graph, &a.A)) return rc;
    if (int rc = fr_children(h, who, pb, pool->n_graph, &a.B)) return rc;
  }
  a.K = j.n; a.m = M; a.sel_rows = sel_rows; a.sel_slots = sel_slots; a.sel_dec = sel_decisions; a.gnn_dec = gnn_decisions; a.gnn_imp = gnn_improvement;
  a.ineff = ineff; a.kw_imp = kw_improvement; a.used = used_kw; a.dec = decisions;
  hipStream_t st = (hipStream_t)stream;
  Launcher run{h, st};
  run.run(PC_FR_CHOOSE_JOBS, [&] { hipLaunchKernelGGL(k_frontier_choose_jobs, dim3(j.n_entries), dim3(FR_THREADS), 0, st, a, j, m_entry); });
  if (M > 0) run.run(PC_FR_CHOOSE_COPY, [&] { hipLaunchKernelGGL(k_frontier_choose_copy, dim3(2 * M, FR_SPLIT), dim3(FR_THREADS), 0, st, a); });
  return run.rc;
}

// ---- BaBSR alone: the decision of every parent row (reference plnn/relu_conv_any_kw.py:45-181, the decision
// rule of plnn/kw_score_conv.py:115-156) ----
extern "C" size_t gnnb_frontier_babsr_decide_workspace_bytes(const gnnb_t* h, int K) {
  if (!h || !h->bound || K < 1) return 0;
  return (size_t)K * FC_COUNT * sizeof(int32_t);
}

// The checks gnnb_frontier_babsr_decide and gnnb_frontier_babsr_decide_jobs share on the rule's own arguments, before the handle is looked
// at (as K's range is), and the arguments of k_frontier_candidates / fr_fallback_walk without a pair A.
static int fr_babsr_ranges(const char* who, int n_order, double decision_threshold) {
  if (n_order < 0 || n_order > MAXL) return fail(GNNB_E_INVALID, "%s: random_order of n_order = %d layers (0..%d)", who, n_order, MAXL);
  if (decision_threshold != decision_threshold) return fail(GNNB_E_INVALID, "%s: decision_threshold = %g", who, decision_threshold);
  return GNNB_OK;
}

static int fr_babsr_args(const gnnb_t* h, const char* who, int n, const float* scores, const float* intercepts, const float* scorer_mask,
                         double decision_threshold, int sparsest_layer, const int32_t* random_order, int n_order, int32_t* icp, int32_t* decisions,
                         void* workspace, size_t workspace_bytes, FrFallbackArgs* a) {
  if (!scores || !intercepts || !scorer_mask || !icp || !decisions || !workspace || (n_order > 0 && !random_order))
    return fail(GNNB_E_INVALID, "%s: null argument", who);
  const size_t need = (size_t)n * FC_COUNT * sizeof(int32_t);
  if (workspace_bytes < need) return fail(GNNB_E_NOMEM, "%s: workspace %zu bytes, need %zu", who, workspace_bytes, need);
  a->s = fr_shape(h);
  a->K = n; a->scores = scores; a->icp_tb = intercepts; a->amb = scorer_mask;
  a->decision_threshold = decision_threshold; a->sparsest_layer = sparsest_layer; a->n_order = n_order;
  for (int q = 0; q < n_order; ++q) a->order[q] = random_order[q];
  a->icp = icp; a->kw_dec = decisions; a->cand = (int32_t*)workspace; a->pair_a = 0;
  return GNNB_OK;
}

extern "C" int gnnb_frontier_babsr_decide(gnnb_t* h, int K, const float* scores, const float* intercepts, const float* scorer_mask,
                                          double decision_threshold, int sparsest_layer, const int32_t* random_order, int n_order, int32_t* icp,
                                          int32_t* decisions, void* workspace, size_t workspace_bytes, void* stream) {
  const char* who = "gnnb_frontier_babsr_decide";
  if (K < 1 || K > 32767) return fail(GNNB_E_INVALID, "%s: K = %d outside 1..32767", who, K);
  if (int rc = fr_babsr_ranges(who, n_order, decision_threshold)) return rc;
  if (int rc = net_preflight(h, who)) return rc;
  FrFallbackArgs a{};
  if (int rc = fr_babsr_args(h, who, K, scores, intercepts, scorer_mask, decision_threshold, sparsest_layer, random_order, n_order, icp, decisions,
                             workspace, workspace_bytes, &a))
    return rc;
  hipStream_t st = (hipStream_t)stream;
  Launcher run{h, st};
  run.run(PC_FR_CANDIDATES, [&] { hipLaunchKernelGGL(k_frontier_candidates, dim3(K), dim3(FR_THREADS), 0, st, a); });
  run.run(PC_FR_BABSR_DECIDE, [&] { hipLaunchKernelGGL(k_frontier_babsr_decide, dim3(1), dim3(64), 0, st, a); });
  return run.rc;
}

extern "C" int gnnb_frontier_babsr_decide_jobs(gnnb_t* h, const gnnb_plan* plan, const float* scores, const float* intercepts,
                                               const float* scorer_mask, double decision_threshold, int sparsest_layer, const int32_t* random_order,
                                               int n_order, int32_t* icp, int32_t* decisions, void* workspace, size_t workspace_bytes, void* stream) {
  const char* who = "gnnb_frontier_babsr_decide_jobs";
  if (int rc = fr_babsr_ranges(who, n_order, decision_threshold)) return rc;
  FrPlan j{};
  const int ng = h && h->bound ? h->kw_net.L + 2 : 0;
  if (int rc = fr_plan(h, who, plan, &ng, &j)) return rc;
  FrFallbackArgs a{};
  if (int rc = fr_babsr_args(h, who, j.n, scores, intercepts, scorer_mask, decision_threshold, sparsest_layer, random_order, n_order, icp, decisions,
                             workspace, workspace_bytes, &a))
    return rc;
  hipStream_t st = (hipStream_t)stream;
  Launcher run{h, st};
  run.run(PC_FR_CANDIDATES, [&] { hipLaunchKernelGGL(k_frontier_candidates, dim3(j.n), dim3(FR_THREADS), 0, st, a); });
  run.run(PC_FR_BABSR_DECIDE_JOBS, [&] { hipLaunchKernelGGL(k_frontier_babsr_decide_jobs, dim3(j.n_entries), dim3(64), 0, st, a, j); });
  return run.rc;
}

// ---- strong branching (gnnb_k_strong.h): the candidates of every parent row, and the best of them ----
extern "C" size_t gnnb_strong_list_workspace_bytes(const gnnb_t* h, int K) {
  if (!h || !h->bound || K < 1) return 0;
  return (size_t)K * SC_FIELDS * sizeof(int32_t);
}

extern "C" int gnnb_strong_list(gnnb_t* h, const gnnb_pool* pool, const int32_t* slots, int K, const float* scorer_mask, const float* scores,
                                int top_m, int32_t* cand0, int32_t* cand_row, int32_t* cand_slot, int32_t* cand_dec, void* workspace,
                                size_t workspace_bytes, void* stream) {
  const char* who = "gnnb_strong_list";
  if (K < 1 || K > 32767) return fail(GNNB_E_INVALID, "%s: K = %d outside 1..32767", who, K);
  if (top_m < 0) return fail(GNNB_E_INVALID, "%s: top_m = %d (0: every undecided node, or the number of candidates per row)", who, top_m);
  if (top_m > 0 && !scores) return fail(GNNB_E_INVALID, "%s: top_m = %d needs scores (null)", who, top_m);
  if (int rc = frontier_preflight(h, who, K, pool ? &pool->n_graph : nullptr)) return rc;
  if (!slots || !scorer_mask || !cand0 || !cand_row || !cand_slot || !cand_dec || !workspace) return fail(GNNB_E_INVALID, "%s: null argument", who);
  const size_t need = gnnb_strong_list_workspace_bytes(h, K);
  if (workspace_bytes < need) return fail(GNNB_E_NOMEM, "%s: workspace %zu bytes, need %zu", who, workspace_bytes, need);
  StrongListArgs a{};
  a.s = fr_shape(h);
  if (int rc = fr_pool(h, who, pool, &a.p)) return rc;
  a.slots = slots; a.K = K; a.amb = scorer_mask; a.scores = scores; a.top_m = top_m;
  a.cand0 = cand0; a.cand_row = cand_row; a.cand_slot = cand_slot; a.cand_dec = cand_dec; a.rows = (int32_t*)workspace;
  hipStream_t st = (hipStream_t)stream;
  Launcher run{h, st};
  run.run(PC_STRONG_COUNT, [&] { hipLaunchKernelGGL(k_strong_count, dim3(K), dim3(FR_THREADS), 0, st, a); });
  run.run(PC_STRONG_COMPACT, [&] { hipLaunchKernelGGL(k_strong_compact, dim3(K), dim3(FR_THREADS), 0, st, a); });
  return run.rc;
}

// ---- the union of two shortlists: k_strong_count per array, then the union's count and its compaction ----
extern "C" size_t gnnb_strong_list_union_workspace_bytes(const gnnb_t* h, int K) {
  if (!h || !h->bound || K < 1) return 0;
  return (size_t)K * (2 * SC_FIELDS + 1) * sizeof(int32_t);   // both arrays' records and the rows' union counts
}

extern "C" int gnnb_strong_list_union(gnnb_t* h, const gnnb_pool* pool, const int32_t* slots, int K, const float* scorer_mask,
                                      const float* scores_a, int top_a, const float* scores_b, int top_b, int32_t* cand0, int32_t* cand_row,
                                      int32_t* cand_slot, int32_t* cand_dec, int32_t* cand_src, void* workspace, size_t workspace_bytes,
                                      void* stream) {
  const char* who = "gnnb_strong_list_union";
  if (K < 1 || K > 32767) return fail(GNNB_E_INVALID, "%s: K = %d outside 1..32767", who, K);
  if (top_a < 1 || top_b < 1)
    return fail(GNNB_E_INVALID, "%s: top_a = %d , top_b = %d (both at least 1; one list alone is gnnb_strong_list)", who, top_a, top_b);
  if (int rc = frontier_preflight(h, who, K, pool ? &pool->n_graph : nullptr)) return rc;
  if (!slots || !scorer_mask || !scores_a || !scores_b || !cand0 || !cand_row || !cand_slot || !cand_dec || !cand_src || !workspace)
    return fail(GNNB_E_INVALID, "%s: null argument", who);
  const size_t need = gnnb_strong_list_union_workspace_bytes(h, K);
  if (workspace_bytes < need) return fail(GNNB_E_NOMEM, "%s: workspace %zu bytes, need %zu", who, workspace_bytes, need);
  StrongListArgs ca{};
  ca.s = fr_shape(h);
  if (int rc = fr_pool(h, who, pool, &ca.p)) return rc;
  int32_t* ws = (int32_t*)workspace;
  ca.slots = slots; ca.K = K; ca.amb = scorer_mask; ca.scores = scores_a; ca.top_m = top_a; ca.rows = ws;
  StrongListArgs cb = ca;
  cb.scores = scores_b; cb.top_m = top_b; cb.rows = ws + (size_t)K * SC_FIELDS;
  StrongUnionArgs u{};
  u.s = ca.s; u.slots = slots; u.K = K; u.amb = scorer_mask; u.scores_a = scores_a; u.scores_b = scores_b;
  u.cand0 = cand0; u.cand_row = cand_row; u.cand_slot = cand_slot; u.cand_dec = cand_dec; u.cand_src = cand_src;
  u.rows_a = ca.rows; u.rows_b = cb.rows; u.count = ws + (size_t)K * 2 * SC_FIELDS;
  hipStream_t st = (hipStream_t)stream;
  Launcher run{h, st};
  run.run(PC_STRONG_COUNT, [&] { hipLaunchKernelGGL(k_strong_count, dim3(K), dim3(FR_THREADS), 0, st, ca); });
  run.run(PC_STRONG_COUNT, [&] { hipLaunchKernelGGL(k_strong_count, dim3(K), dim3(FR_THREADS), 0, st, cb); });
  run.run(PC_STRONG_COUNT, [&] { hipLaunchKernelGGL(k_strong_union_count, dim3(K), dim3(FR_THREADS), 0, st, u); });
  run.run(PC_STRONG_COMPACT, [&] { hipLaunchKernelGGL(k_strong_union_compact, dim3(K), dim3(FR_THREADS), 0, st, u); });
  return run.rc;
}

extern "C" int gnnb_strong_pick(gnnb_t* h, const gnnb_pool* pool, const int32_t* slots, int K, const int32_t* cand0, const int32_t* cand_dec,
                                const int32_t* live, const int32_t* infeasible, const double* bound, int32_t* decisions,
                                double* best_improvement, double* improvement, double* table, void* stream) {
  const char* who = "gnnb_strong_pick";
  if (int rc = frontier_preflight(h, who, K, pool ? &pool->n_graph : nullptr)) return rc;
  if (!slots || !cand0 || !cand_dec || !live || !infeasible || !bound || !decisions || !best_improvement || !improvement)
    return fail(GNNB_E_INVALID, "%s: null argument", who);
  StrongPickArgs a{};
  a.s = fr_shape(h);
  if (int rc = fr_pool(h, who, pool, &a.p)) return rc;
  a.slots = slots; a.K = K; a.cand0 = cand0; a.cand_dec = cand_dec; a.live = live; a.infeasible = infeasible; a.bound = bound;
  a.decisions = decisions; a.best = best_improvement; a.imp = improvement; a.table = table;
  hipStream_t st = (hipStream_t)stream;
  Launcher run{h, st};
  run.run(PC_STRONG_PICK, [&] { hipLaunchKernelGGL(k_strong_pick, dim3(K), dim3(FR_THREADS), 0, st, a); });
  return run.rc;
}

// ---- strong branching for many jobs in one pool: the candidates' boxes and property rows, by the segment of
// their slot.  The copy is k_frontier_rows_sel's and launches under its class: no profile class was added ----
extern "C" int gnnb_strong_rows_jobs(gnnb_t* h, const int32_t* cand_slot, int c, int segments, int seg_cap, const double* seg_x_lo,
                                     const double* seg_x_hi, const float* seg_prop_w, const float* seg_prop_b, double* x_lo, double* x_hi,
                                     float* prop_w, float* prop_b, void* stream) {
  const char* who = "gnnb_strong_rows_jobs";
  if (c < 1 || c > 32767) return fail(GNNB_E_INVALID, "%s: c = %d outside 1..32767", who, c);
  if (segments < 1 || seg_cap < 1) return fail(GNNB_E_INVALID, "%s: segments = %d of seg_cap = %d slots (both at least 1)", who, segments, seg_cap);
  if (int rc = net_preflight(h, who)) return rc;
  if (!cand_slot || !seg_x_lo || !seg_x_hi || !seg_prop_w || !seg_prop_b || !x_lo || !x_hi || !prop_w || !prop_b)
    return fail(GNNB_E_INVALID, "%s: null argument", who);
  StrongRowsArgs a{};
  a.cand_slot = cand_slot; a.c = c; a.S = segments; a.seg_cap = seg_cap;
  a.r = FrSegRows{h->kw_net.N[0], h->kw_net.N[h->kw_net.L], seg_x_lo, seg_x_hi, seg_prop_w, seg_prop_b, x_lo, x_hi, prop_w, prop_b};
  hipStream_t st = (hipStream_t)stream;
  Launcher run{h, st};
  run.run(PC_FR_ROWS_SEL, [&] { hipLaunchKernelGGL(k_strong_rows_jobs, dim3(2 * c, FR_SPLIT), dim3(FR_THREADS), 0, st, a); });
  return run.rc;
}

// ---- the learn rows of an online round (reference plnn/relu_conv_online.py:183-207) ----
extern "C" int gnnb_frontier_learn(gnnb_t* h, int K, const int32_t* gnn_decisions, const int32_t* kw_decisions, const int32_t* used_kw,
                                   const double* gnn_improvement, const double* kw_improvement, int online_threshold, int32_t* wrong,
                                   int32_t* learn_rows, int32_t* learn_kw, float* learn_imp, int32_t* n_learn, void* stream) {
  const char* who = "gnnb_frontier_learn";
  const int ng = h && h->bound ? h->kw_net.L + 2 : 0;
  if (int rc = frontier_preflight(h, who, K, &ng)) return rc;
  if (online_threshold < 1) return fail(GNNB_E_INVALID, "%s: online_threshold = %d (>= 1)", who, online_threshold);
  if (!gnn_decisions || !kw_decisions || !used_kw || !gnn_improvement || !kw_improvement || !wrong || !learn_rows || !learn_kw || !learn_imp || !n_learn)
    return fail(GNNB_E_INVALID, "%s: null argument", who);
  FrLearnArgs a{};
  a.s = fr_shape(h);
  a.K = K; a.gnn_dec = gnn_decisions; a.kw_dec = kw_decisions; a.used = used_kw; a.gnn_imp = gnn_improvement; a.kw_imp = kw_improvement;
  a.online_threshold = online_threshold;
  a.wrong = wrong; a.learn_rows = learn_rows; a.learn_kw = learn_kw; a.learn_imp = learn_imp; a.n_learn = n_learn;
  hipStream_t st = (hipStream_t)stream;
  Launcher run{h, st};
  run.run(PC_FR_LEARN, [&] { hipLaunchKernelGGL(k_frontier_learn, dim3(1), dim3(64), 0, st, a); });
  return run.rc;
}

// ---- the learn rows of every job of a many-jobs online round: the walk above per plan entry on the segment's
// table wrong[segment]; the learn rows of all entries form one dense list in plan order ----
struct FrLearnWs { size_t st_kw, st_imp, n_stage, total; };              // byte offsets in gnnb_frontier_learn_jobs' workspace: the staged rows at 0
static FrLearnWs fr_learn_ws_layout(int n) {
  const auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
  FrLearnWs w;
  w.st_kw = up((size_t)n * sizeof(int32_t));
  w.st_imp = w.st_kw + up((size_t)n * sizeof(int32_t));
  w.n_stage = w.st_imp + up((size_t)n * sizeof(float));
  w.total = w.n_stage + up((size_t)n * sizeof(int32_t));                 // (an entry holds at least one row: n_entries <= n)
  return w;
}

extern "C" size_t gnnb_frontier_learn_jobs_workspace_bytes(const gnnb_t* h, int n) {
  if (!h || !h->bound || n < 1) return 0;
  return fr_learn_ws_layout(n).total;
}

extern "C" int gnnb_frontier_learn_jobs(gnnb_t* h, const gnnb_plan* plan, const int32_t* gnn_decisions, const int32_t* kw_decisions,
                                        const int32_t* used_kw, const double* gnn_improvement, const double* kw_improvement, int online_threshold,
                                        int32_t* wrong, int32_t* learn_rows, int32_t* learn_kw, float* learn_imp, int32_t* learn_entry,
                                        void* workspace, size_t workspace_bytes, void* stream) {
  const char* who = "gnnb_frontier_learn_jobs";
  FrLearnSelArgs sel{};
  const int ng = h && h->bound ? h->kw_net.L + 2 : 0;
  if (int rc = fr_plan(h, who, plan, &ng, &sel.j)) return rc;
  if (online_threshold < 1) return fail(GNNB_E_INVALID, "%s: online_threshold = %d (>= 1)", who, online_threshold);
  if (!gnn_decisions || !kw_decisions || !used_kw || !gnn_improvement || !kw_improvement || !wrong || !learn_rows || !learn_kw || !learn_imp ||
      !learn_entry || !workspace)
    return fail(GNNB_E_INVALID, "%s: null argument", who);
  const int n = sel.j.n;
  const FrLearnWs ws = fr_learn_ws_layout(n);
  if (workspace_bytes < ws.total) return fail(GNNB_E_NOMEM, "%s: workspace %zu bytes, need %zu", who, workspace_bytes, ws.total);
  char* w = (char*)workspace;
  int32_t* n_stage = (int32_t*)(w + ws.n_stage);
  FrLearnArgs a{};
  a.s = fr_shape(h);
  a.K = n; a.gnn_dec = gnn_decisions; a.kw_dec = kw_decisions; a.used = used_kw; a.gnn_imp = gnn_improvement; a.kw_imp = kw_improvement;
  a.online_threshold = online_threshold;
  a.wrong = wrong; a.learn_rows = (int32_t*)w; a.learn_kw = (int32_t*)(w + ws.st_kw); a.learn_imp = (float*)(w + ws.st_imp); a.n_learn = nullptr;
  sel.n_stage = n_stage; sel.st_rows = a.learn_rows; sel.st_kw = a.learn_kw; sel.st_imp = a.learn_imp;
  sel.learn_rows = learn_rows; sel.learn_kw = learn_kw; sel.learn_imp = learn_imp; sel.learn_entry = learn_entry;
  const FrPlan j = sel.j;
  hipStream_t st = (hipStream_t)stream;
  Launcher run{h, st};
  run.run(PC_FR_LEARN, [&] { hipLaunchKernelGGL(k_frontier_learn_jobs, dim3(j.n_entries), dim3(64), 0, st, a, j, n_stage); });
  run.run(PC_FR_LEARN, [&] { hipLaunchKernelGGL(k_frontier_learn_compact, dim3(1), dim3(FR_THREADS), 0, st, sel); });
  return run.rc;
}

// ---- the witness of the upper bound (reference plnn/branch_and_bound.py:157 global_ub_point) ----
// The checks gnnb_frontier_witness and gnnb_frontier_witness_jobs share on the children and a gnnb_witness_src over n parents, m of them selected.
static int fr_witness_in(const gnnb_t* h, const char* who, int n, int m, const gnnb_children* ch, const gnnb_witness_src* src, double* best_value,
                         float* best_point, FrWitnessArgs* a) {
  if (!ch || !src || !best_value || !best_point || !src->x_a) return fail(GNNB_E_INVALID, "%s: null argument", who);
  if (src->used_kw && m > 0 && (!src->x_b || !src->sel_rows)) return fail(GNNB_E_INVALID, "%s: used_kw with m = %d needs x_b and sel_rows", who, m);
  FrChildrenRO rows{};
  if (int rc = fr_children(h, who, ch, h->kw_net.L + 2, &rows)) return rc;
  a->N0 = h->kw_net.N[0];
  a->live = rows.live; a->infeasible = rows.infeasible; a->ubv = rows.ubv;
  a->x_a = src->x_a; a->x_b = src->x_b;
  a->used = m > 0 ? src->used_kw : nullptr; a->sel_rows = src->sel_rows;      // (without a selected parent no row is pair B's)
  a->K = n; a->m = m;
  a->best_value = best_value; a->best_point = best_point;
  return GNNB_OK;
}

extern "C" int gnnb_frontier_witness(gnnb_t* h, int K, const gnnb_children* children, const gnnb_witness_src* src, double* best_value,
                                     float* best_point, void* stream) {
  const char* who = "gnnb_frontier_witness";
  if (K < 1 || K > 32767) return fail(GNNB_E_INVALID, "%s: K = %d outside 1..32767", who, K);
  if (src && (src->m < 0 || src->m > K)) return fail(GNNB_E_INVALID, "%s: m = %d selected parents of K = %d", who, src->m, K);
  const int ng = h && h->bound ? h->kw_net.L + 2 : 0;
  size_t lds = 0;
  if (int rc = kw_preflight(h, who, &ng, &lds)) return rc;
  FrWitnessArgs a{};
  if (int rc = fr_witness_in(h, who, K, src ? src->m : 0, children, src, best_value, best_point, &a)) return rc;
  hipStream_t st = (hipStream_t)stream;
  Launcher run{h, st};
  run.run(PC_FR_WITNESS, [&] { hipLaunchKernelGGL(k_frontier_witness, dim3(1), dim3(FR_THREADS), 0, st, a); });
  return run.rc;
}

extern "C" int gnnb_frontier_witness_jobs(gnnb_t* h, const gnnb_plan* plan, int M, const int32_t* m_entry, const gnnb_children* children,
                                          const gnnb_witness_src* src, double* best_value, float* best_point, void* stream) {
  const char* who = "gnnb_frontier_witness_jobs";
  FrPlan j{};
  if (plan && plan->n >= 1 && plan->n <= 32767 && (M < 0 || M > plan->n))      // (as K's range: before the handle is looked at)
    return fail(GNNB_E_INVALID, "%s: M = %d selected parents of n = %d", who, M, plan->n);
  const int ng = h && h->bound ? h->kw_net.L + 2 : 0;
  if (int rc = fr_plan(h, who, plan, &ng, &j)) return rc;
  if (M < 0 || M > j.n) return fail(GNNB_E_INVALID, "%s: M = %d selected parents of n = %d", who, M, j.n);
  if (M > 0 && src && src->used_kw && !m_entry) return fail(GNNB_E_INVALID, "%s: null m_entry with M = %d", who, M);
  FrWitnessArgs a{};
  if (int rc = fr_witness_in(h, who, j.n, M, children, src, best_value, best_point, &a)) return rc;
  hipStream_t st = (hipStream_t)stream;
  Launcher run{h, st};
  run.run(PC_FR_WITNESS_JOBS, [&] { hipLaunchKernelGGL(k_frontier_witness_jobs, dim3(j.n_entries), dim3(FR_THREADS), 0, st, a, j, m_entry); });
  return run.rc;
}


// ================================================================================================================
// Online learning (reference graphnet/graph_score_online.py:9-23, :62-77)
// ================================================================================================================
// The device pack builder: the packs from the trainer's d_w, in place, on `st` (k_repack_fold, k_repack_emit).  Allocates nothing and
// does not synchronise.
static int repack_device(gnnb_t* h, hipStream_t st) {
  const float* d_w = h->trainer->d_w.get();
  float* scr = h->repack_scr.get();
  hipLaunchKernelGGL(k_repack_fold, dim3((kFoldJobElems + kRepackBlock - 1) / kRepackBlock, kFoldJobs), dim3(kRepackBlock), 0, st, d_w, scr);
  hipLaunchKernelGGL(k_repack_emit, dim3((unsigned)h->repack_nblocks), dim3(kRepackBlock), 0, st, h->repack_segs.get(), h->repack_nseg, d_w,
                     (const float*)scr, h->pack_block.get());
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(GNNB_E_HIP, "launch of k_repack_fold / k_repack_emit failed: %s", hipGetErrorString(e));
  return GNNB_OK;
}
// h->blob as the trainer's d_w has it: a step in repack mode 1 leaves the host copy behind (every reader of h->blob calls this first)
static int fresh_blob(gnnb_t* h) {
  if (!h->blob_stale) return GNNB_OK;
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipMemcpy(h->blob.data(), h->trainer->d_w.get(), blob_floats() * sizeof(float), hipMemcpyDeviceToHost));
  h->blob_stale = false;
  return GNNB_OK;
}

extern "C" int gnnb_get_weights(const gnnb_t* h, float* w_blob, size_t n_floats) {
  if (!h || !w_blob) return fail(GNNB_E_INVALID, "gnnb_get_weights: null argument");
  if (n_floats != blob_floats()) return fail(GNNB_E_INVALID, "gnnb_get_weights: %zu floats, expected %zu", n_floats, blob_floats());
  if (int rc = fresh_blob(const_cast<gnnb_t*>(h))) return rc;
  memcpy(w_blob, h->blob.data(), n_floats * sizeof(float));
  return GNNB_OK;
}

extern "C" int gnnb_set_weights(gnnb_t* h, const float* w_blob, size_t n_floats) {
  if (!h || !w_blob) return fail(GNNB_E_INVALID, "gnnb_set_weights: null argument");
  if (n_floats != blob_floats()) return fail(GNNB_E_INVALID, "gnnb_set_weights: %zu floats, expected %zu", n_floats, blob_floats());
  HIPCHK(hipDeviceSynchronize());          // no forward may still be reading the packs
  if (h->trainer && h->repack_mode == 1) {      // the packs come from the mode's builder: blob to d_w, then the device builder
    h->blob.assign(w_blob, w_blob + n_floats);
    h->blob_stale = false;
    HIPCHK(hipMemcpy(h->trainer->d_w.get(), w_blob, n_floats * sizeof(float), hipMemcpyHostToDevice));
    if (int rc = repack_device(h, nullptr)) return rc;
    HIPCHK(hipStreamSynchronize(nullptr));
    return GNNB_OK;
  }
  if (int rc = load_weights(h, w_blob, nullptr)) return rc;
  if (h->trainer) HIPCHK(hipMemcpy(h->trainer->d_w.get(), w_blob, n_floats * sizeof(float), hipMemcpyHostToDevice));
  return GNNB_OK;
}

// Which builder rebuilds the packs after a learning step: 0 (default) build_packs on the host, 1 the device builder on the step's stream.
extern "C" int gnnb_online_set_repack(gnnb_t* h, int mode) {
  if (!h) return fail(GNNB_E_INVALID, "gnnb_online_set_repack: null handle");
  if (!h->trainer) return fail(GNNB_E_STATE, "gnnb_online_set_repack: no trainer (gnnb_online_create)");
  if (mode != 0 && mode != 1) return fail(GNNB_E_INVALID, "gnnb_online_set_repack: mode = %d (0: host builder, 1: device builder)", mode);
  if (mode == h->repack_mode) return GNNB_OK;
  HIPCHK(hipDeviceSynchronize());          // no forward may still be reading the packs
  if (mode == 1) {
    if (int rc = repack_device(h, nullptr)) return rc;
    HIPCHK(hipStreamSynchronize(nullptr));
  } else {
    if (int rc = fresh_blob(h)) return rc;
    const std::vector<float> w(h->blob);
    if (int rc = load_weights(h, w.data(), nullptr)) return rc;
  }
  h->repack_mode = mode;
  return GNNB_OK;
}

extern "C" int gnnb_repack(gnnb_t* h, void* stream) {
  if (!h) return fail(GNNB_E_INVALID, "gnnb_repack: null handle");
  if (!h->trainer) return fail(GNNB_E_STATE, "gnnb_repack: no trainer (gnnb_online_create)");
  return repack_device(h, (hipStream_t)stream);
}

// Inspection: every float of the pack block becomes a NaN (tests: a builder that runs next has to write them all).  Device-synchronising.
extern "C" int gnnb_debug_poison_packs(gnnb_t* h) {
  if (!h) return fail(GNNB_E_INVALID, "gnnb_debug_poison_packs: null handle");
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipMemset(h->pack_block.get(), 0xff, h->pack_block.size() * sizeof(float)));
  HIPCHK(hipDeviceSynchronize());
  return GNNB_OK;
}

// Inspection: pack `which` (0..13: embed, pre_fwd, pre_bwd, pre_inp, prop, upd_fwd_e, upd_fwd_i, upd_fwd_f, upd_bwd, upd_bwd_b, upd_inp,
// post_inp, score_b, score_f) as it stands in device memory, after a device synchronise.
extern "C" int gnnb_pack_image(const gnnb_t* h, int which, float* host_buf, size_t cap, size_t* n_floats) {
  if (!h) return fail(GNNB_E_INVALID, "gnnb_pack_image: null handle");
  if (which < 0 || which >= N_PACKS) return fail(GNNB_E_INVALID, "gnnb_pack_image: which = %d outside [0, %d)", which, N_PACKS);
  const size_t n = (size_t)kPackFloats[which];
  if (n_floats) *n_floats = n;
  if (!host_buf && cap == 0 && n_floats) return GNNB_OK;      // a size query
  if (!host_buf) return fail(GNNB_E_INVALID, "gnnb_pack_image: null buffer");
  if (cap < n) return fail(GNNB_E_INVALID, "gnnb_pack_image: room for %zu floats, pack %d has %zu", cap, which, n);
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipMemcpy(host_buf, h->d_pack[which], n * sizeof(float), hipMemcpyDeviceToHost));
  return GNNB_OK;
}

#include "gnnb_step.h"      // the learning step: gnnb_online_create .. gnnb_imitation_loss, struct Step, step_tensors and BatchView

// ---- the replay buffer (gnnb_k_replay.h) ----
// What gnnb_replay_push, gnnb_replay_sample and gnnb_replay_bytes share: the capacity's range.
static int refuse_capacity(int C, const char* who) {
  if (C < 1 || C > RP_MAX_CAPACITY) return fail(GNNB_E_INVALID, "%s: C = %d slots (1 <= C <= %d)", who, C, RP_MAX_CAPACITY);
  return GNNB_OK;
}

extern "C" size_t gnnb_replay_bytes(const gnnb_t* h, int C) {
  if (!h || !h->bound || C < 1 || C > RP_MAX_CAPACITY) return 0;
  size_t floats = 2 * (size_t)h->R;                                     // the table's fp64 row
  for (const StepTensor& e : step_tensors(h, h->n_fixed + 1)) floats += (size_t)e.w;
  return (size_t)C * floats * sizeof(float);
}

extern "C" int gnnb_replay_push(gnnb_t* h, const gnnb_batch* src, int K, const double* src_table, const int32_t* rows, int n, const gnnb_batch* dst,
                                int C, double* dst_table, int32_t* state, int32_t* status, void* stream) {
  const char* who = "gnnb_replay_push";
  if (int rc = refuse_capacity(C, who)) return rc;
  if (K < 1 || n < 1 || n > K || n > C)
    return fail(GNNB_E_INVALID, "%s: n = %d rows of a batch of K = %d into C = %d slots (1 <= n <= K, n <= C)", who, n, K, C);
  if (!h) return fail(GNNB_E_INVALID, "%s: null handle", who);
  if (!src || !src_table || !rows || !dst || !dst_table || !state) return fail(GNNB_E_INVALID, "%s: null argument", who);
  if (!h->bound) return fail(GNNB_E_STATE, "%s: call gnnb_bind_network first", who);
  if (int rc = refuse_batch(h, src, K, kNeedsOnline, who)) return rc;
  if (int rc = refuse_batch(h, dst, C, kNeedsOnline, who)) return rc;
  if (src->n_primal != dst->n_primal)
    return fail(GNNB_E_INVALID, "%s: the source batch has %d primal tensors, the buffer %d", who, src->n_primal, dst->n_primal);
  const int L = (int)h->N.size() - 2, R = h->R;
  if (L > T_MAXL) return fail(GNNB_E_INVALID, "%s: more than %d ReLU layers", who, T_MAXL);
  hipStream_t st = (hipStream_t)stream;
  if (h->replay_slot.size() < (size_t)n) HIPCHK(h->replay_slot.alloc((size_t)(n < 1024 ? 1024 : n)));
  ReplayStore g{};
  g.rows = rows; g.slot = h->replay_slot.get();
  for (const StepTensor& e : step_tensors(h, src->n_primal))
    g.t[g.nt++] = gnnb_train::TGatherT{step_tensor(*src, e), const_cast<float*>(step_tensor(*dst, e)), (int)e.w};
  g.t[g.nt++] = gnnb_train::TGatherT{reinterpret_cast<const float*>(src_table), reinterpret_cast<float*>(dst_table), 2 * R};
  ReplayRank a{src_table, src->mask, rows, n, K, R, C, h->replay_slot.get(), state, status};
  hipLaunchKernelGGL(k_replay_rank, dim3(1), dim3(RP_THREADS), 0, st, a);
  hipLaunchKernelGGL(k_replay_store, dim3(n, TG_SPLIT), dim3(TG_THREADS), 0, st, g);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(GNNB_E_HIP, "%s: a launch failed: %s", who, hipGetErrorString(e));
  return GNNB_OK;
}

extern "C" int gnnb_replay_sample(gnnb_t* h, const int32_t* state, int C, int n, uint64_t seed, uint64_t draw, int32_t* idx, void* stream) {
  const char* who = "gnnb_replay_sample";
  if (int rc = refuse_capacity(C, who)) return rc;
  if (n < 1 || n > RP_MAX_SAMPLE) return fail(GNNB_E_INVALID, "%s: n = %d slots (1 <= n <= %d)", who, n, RP_MAX_SAMPLE);
  if (!h) return fail(GNNB_E_INVALID, "%s: null handle", who);
  if (!state || !idx) return fail(GNNB_E_INVALID, "%s: null argument", who);
  ReplaySample a{state, C, n, (unsigned long long)seed, (unsigned long long)draw, idx};
  hipLaunchKernelGGL(k_replay_sample, dim3(1), dim3(RP_THREADS), 0, (hipStream_t)stream, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(GNNB_E_HIP, "%s: the launch failed: %s", who, hipGetErrorString(e));
  return GNNB_OK;
}
