// Online-learning step of the branching GNN on the device: its host side, the tape.
//
// Reference: graphnet/graph_score_online.py:62-77 (GraphChoice.online_learning) --
//     loss = gnn_score - kw_score + improvement;  loss.backward();  Adam(lr, weight_decay).step()
// where gnn_score = max of the scores of one subproblem and kw_score = the score of the node the BaBSR heuristic chose
// (relu_conv_online.py:58-276 calls it once per branch whose KW decision beat the GNN's).  torch.autograd does the backward
// pass there; here the forward of graph_conv.py:77-388 / :442-470 is re-run in "training form" -- every Linear of the GNN as
// its own kernel with its output kept -- on a tape, then the tape is walked backwards with hand-written adjoint kernels, and
// one Adam kernel updates the 117 825 parameters in place.  The scorer's fused inference kernels are not used here: their
// folded weight packs are rebuilt from the new parameters after the step.
//
// Three files: gnnb_k_train.h holds the kernels and their argument structs (and what there is to say about their precision); this one
// the arena, the `Trainer` -- the parameters, the tape, and the builders that put a chain of Linears or an edge on it -- and the one
// place that picks a chain kernel's tile height; gnnb_step.h the step itself (`struct Step`, stage by stage) and its entry points.
//
// Included by gnnb.hip (one translation unit: it uses the bound network of gnnb_handle) behind gnnb_mem.h, whose owners hold its memory.
#pragma once
#include <functional>
#include "gnnb_k_train.h"

namespace gnnb_train {
using namespace gnnb;

// ---- device memory: a bump arena, zeroed at the start of every step (gradient buffers start at 0) ----
struct Arena {
  struct Chunk { DevBuf<char> p; size_t used; };      // (released with the arena)
  std::vector<Chunk> chunks;
  size_t chunk_bytes = (size_t)256 << 20;
  int err = 0;
  float* alloc(size_t nfloats) {
    const size_t bytes = (nfloats * 4 + 255) & ~(size_t)255;
    for (auto& c : chunks)
      if (c.p.size() - c.used >= bytes) { float* r = (float*)(c.p.get() + c.used); c.used += bytes; return r; }
    Chunk c{{}, bytes};
    const size_t cap = bytes > chunk_bytes ? bytes : chunk_bytes;
    if (c.p.alloc(cap) != hipSuccess || hipMemset(c.p.get(), 0, cap) != hipSuccess) { err = 1; return nullptr; }
    chunks.push_back(std::move(c));
    return (float*)chunks.back().p.get();
  }
  int reset(hipStream_t st) {          // everything handed out so far back to zero, arena empty
    for (auto& c : chunks) {
      if (c.used && hipMemsetAsync(c.p.get(), 0, c.used, st) != hipSuccess) return 1;
      c.used = 0;
    }
    return 0;
  }
};

struct TT { float* v = nullptr; float* g = nullptr; long n = 0; };   // rows (n, 64): value and gradient

// ---- the tile height of a chain launch, and the kernels by it ----
// Few rows (the latency case: one subproblem has ~1000 live nodes per layer): 4-row tiles -- eight times the blocks, each an eighth of
// the inner loop, the weights staged per block either way (base B = 1, ms per step: 32-row tiles 3.31, 16: 2.64, 8: 2.56, 4: 2.21); a few
// thousand rows: 8-row tiles; many rows: 32-row tiles amortise the staging.
enum { TILE_FORMS = 3 };
inline int tile_rows(long nrows, int n_cu) { return nrows <= 16L * n_cu ? TL_ROWS_TINY : (nrows <= 128L * n_cu ? TL_ROWS_SMALL : TL_ROWS); }
inline int tile_form(int R) { return R == TL_ROWS_TINY ? 0 : (R == TL_ROWS_SMALL ? 1 : 2); }      // index into the kernel tables below
// dynamic LDS of a forward chain kernel at R rows per tile: Ws [64][Kmax | 1], Xs [R][Kmax], Ys [R][64]
inline size_t tile_lds_bytes(int R, int Kmax) { return ((size_t)(Kmax | 1) * 64 + (size_t)R * Kmax + (size_t)R * 64) * 4; }
static void (*const kChainFwd[TILE_FORMS])(TChain) = {k_tchain_fwd<TL_ROWS_TINY>, k_tchain_fwd<TL_ROWS_SMALL>, k_tchain_fwd<TL_ROWS>};
static void (*const kChainBwdX[TILE_FORMS])(TChain) = {k_tchain_bwd_x<TL_ROWS_TINY>, k_tchain_bwd_x<TL_ROWS_SMALL>, k_tchain_bwd_x<TL_ROWS>};
static void (*const kChainFwdMulti[TILE_FORMS])(const TChain*) = {k_tchain_fwd_multi<TL_ROWS_TINY>, k_tchain_fwd_multi<TL_ROWS_SMALL>, k_tchain_fwd_multi<TL_ROWS>};
static void (*const kChainBwdXMulti[TILE_FORMS])(const TChain*) = {k_tchain_bwd_x_multi<TL_ROWS_TINY>, k_tchain_bwd_x_multi<TL_ROWS_SMALL>, k_tchain_bwd_x_multi<TL_ROWS>};

// ---- the tape ----
struct Trainer {
  bool ordered = false;                  // the step in flight returns without synchronising: host tables go to the device through k_tput
  int put(void* dst, const void* src, size_t bytes) {      // dst: device memory with room for bytes rounded up to 4
    const unsigned char* s = static_cast<const unsigned char*>(src);
    unsigned* d = static_cast<unsigned*>(dst);
    for (size_t o = 0; o < bytes; o += sizeof(TPutBlock)) {
      TPutBlock b;
      const size_t nb = bytes - o < sizeof(TPutBlock) ? bytes - o : sizeof(TPutBlock);
      memset(b.w, 0, sizeof b.w);
      memcpy(b.w, s + o, nb);
      hipLaunchKernelGGL(k_tput, dim3(1), dim3(256), 0, st, b, d + o / 4, (int)((nb + 3) / 4));
    }
    return hipGetLastError() != hipSuccess;
  }
  int table(void* dst, const void* src, size_t bytes) {    // a host table the kernels of this step read: through k_tput iff `ordered`
    return ordered ? put(dst, src, bytes) : hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, st) != hipSuccess;
  }
  DevBuf<float> d_w, d_g, d_m, d_v;      // parameters (blob order), their gradient, Adam's moments
  int step = 0;
  float lr = 1e-4f, wd = 1e-4f;
  Arena arena;
  std::vector<std::function<void()>> tape;
  hipStream_t st = nullptr;
  int n_cu = 256;
  DevBuf<float> d_scores, d_ds, d_loss, d_imp;      // per batch, grown on demand (gnnb_online_step)
  DevBuf<int> d_kw, d_sel;
  std::vector<float> h_loss;

  TT rows(long n) { TT t; t.n = n; t.v = arena.alloc((size_t)n * 64); t.g = arena.alloc((size_t)n * 64); return t; }

  // a node list: idx (cap) ordered node ids, *cnt their number
  struct List { const int* idx = nullptr; const int* cnt = nullptr; long cap = 0; };

  // One Linear of a chain: y = omask * act(W [segments] + b).  A segment with x == nullptr is the previous op's output.
  struct Segs { TSeg s[3]; int n = 0; Segs(std::initializer_list<TSeg> l = {}) { for (const TSeg& e : l) s[n++] = e; } };
  struct Spec { int layer; Segs segs; const float* feat; bool relu; const float* omask; bool out_full; };
  struct ChainOut { TT t[TC_MAXOPS]; const TT& operator[](int i) const { return t[i]; } };      // the outputs of a chain's ops
  std::vector<TLin> wops;                // every op of the step, in tape (backward) order: the weight-gradient launches walk it

  // THE descriptor builder: a chain of Linears over the same rows (all of them the plain form over n rows, or the compact form over
  // `list`) as the TChain the kernels read, its outputs and partial buffers out of the arena.  list: compact form (rows of an output =
  // list entries, or nodes when its op is out_full); n: rows of the plain form / nodes of the layer.
  struct Built { TChain c{}; ChainOut out; int Kmax = 0; long nrows = 0; };      // Kmax: the largest K of its ops; nrows: rows a launch covers
  Built build(const std::vector<Spec>& specs, long n, const List* list) {
    Built b;
    TChain& c = b.c;
    c.nops = (int)specs.size();
    for (int i = 0; i < c.nops; ++i) {
      const Spec& sp = specs[i];
      TT y = rows(list && !sp.out_full ? list->cap : n);
      TLin& a = c.op[i];
      a.layer = sp.layer;
      a.W = d_w.get() + weight_offset(sp.layer); a.b = d_w.get() + bias_offset(sp.layer);
      a.gW = d_g.get() + weight_offset(sp.layer); a.gb = d_g.get() + bias_offset(sp.layer);
      a.K = kLin[sp.layer].in; a.nseg = sp.segs.n; a.kf = sp.feat ? a.K : 0;
      for (int j = 0; j < a.nseg; ++j) {
        a.seg[j] = sp.segs.s[j];
        if (!sp.segs.s[j].x) {                     // the previous op's output tile
          a.prev |= 1u << j;
          a.seg[j].x = b.out[i - 1].v; a.seg[j].gx = b.out[i - 1].g; a.seg[j].full = specs[i - 1].out_full ? 1 : 0;
        }
      }
      a.feat = sp.feat; a.omask = sp.omask; a.relu = sp.relu ? 1 : 0; a.y = y.v; a.gy = y.g;
      a.n = list ? list->cap : n;
      if (list) { a.ridx = list->idx; a.n_dev = list->cnt; a.out_full = sp.out_full ? 1 : 0; }
      a.nchunks = (int)((a.n + TL_CHUNK - 1) / TL_CHUNK);
      a.part = arena.alloc((size_t)a.nchunks * 64 * (a.K + 1));
      b.Kmax = a.K > b.Kmax ? a.K : b.Kmax;
      b.out.t[i] = y;
    }
    b.nrows = list ? list->cap : n;
    return b;
  }
  static bool wants_gx(const TChain& c) {          // some segment of the chain takes an input gradient
    for (int i = 0; i < c.nops; ++i)
      for (int j = 0; j < c.op[i].nseg; ++j)
        if (c.op[i].seg[j].gx) return true;
    return false;
  }
  void record(const TChain& c) { for (int i = c.nops - 1; i >= 0; --i) wops.push_back(c.op[i]); }

  // One chain: one launch forward, one backward, the descriptor a kernel argument.  Returns the outputs of the ops.
  ChainOut chain(const std::vector<Spec>& specs, long n, const List* list = nullptr) {
    const Built b = build(specs, n, list);
    const int R = tile_rows(b.nrows, n_cu), f = tile_form(R);
    const unsigned nblk = (unsigned)((b.nrows + R - 1) / R);
    hipLaunchKernelGGL(kChainFwd[f], dim3(nblk), dim3(256), tile_lds_bytes(R, b.Kmax), st, b.c);
    tape.push_back([this, c = b.c, nblk, f]() {
      if (wants_gx(c)) hipLaunchKernelGGL(kChainBwdX[f], dim3(nblk), dim3(256), 0, st, c);
      record(c);
    });
    return b.out;
  }
  // Several independent chains (the same chain of different ReLU layers) as ONE launch forward and one backward: blockIdx.y =
  // chain, the descriptors uploaded once and read from memory by both launches.  Returns the outputs per chain.
  struct Job { std::vector<Spec> specs; long n; const List* list; };
  PinnedBuf<TChain> desc;                // pinned, device-visible descriptor slots of the step in flight: read by the kernels where the step ends in a
                                         // sync; an `ordered` step only fills them on the host and its kernels read a device copy (chain_multi)
  int ndesc = 0;
  static constexpr int kDescCap = 8 * T_MAXL;
  std::vector<ChainOut> chain_multi(const std::vector<Job>& jobs) {
    const int nj = (int)jobs.size();
    std::vector<ChainOut> outs(nj);
    TChain* const slots = desc.get();
    if (!slots || ndesc + nj > kDescCap) { arena.err = true; return outs; }
    const TChain* const cs = slots + ndesc;        // (the host reads them again on the way back: they stay until the next step begins)
    long maxrows = 0;
    int Kmax = 0;
    for (int q = 0; q < nj; ++q) {
      const Built b = build(jobs[q].specs, jobs[q].n, jobs[q].list);
      maxrows = b.nrows > maxrows ? b.nrows : maxrows;
      Kmax = b.Kmax > Kmax ? b.Kmax : Kmax;
      slots[ndesc++] = b.c;
      outs[q] = b.out;
    }
    const TChain* d_cs = cs;
    if (ordered) {                       // the pinned slots are rewritten by the next step: this step's kernels read a device copy
      TChain* d = reinterpret_cast<TChain*>(arena.alloc((sizeof(TChain) * nj + 3) / 4));
      if (!d || put(d, cs, sizeof(TChain) * nj)) { arena.err = true; return std::vector<ChainOut>(nj); }
      d_cs = d;
    }
    const int R = tile_rows(maxrows, n_cu), f = tile_form(R);
    const dim3 grid((unsigned)((maxrows + R - 1) / R), (unsigned)nj);
    hipLaunchKernelGGL(kChainFwdMulti[f], grid, dim3(256), tile_lds_bytes(R, Kmax), st, d_cs);
    tape.push_back([this, cs, nj, d_cs, grid, f]() {
      bool any = false;
      for (int q = 0; q < nj; ++q) any = any || wants_gx(cs[q]);
      if (any) hipLaunchKernelGGL(kChainBwdXMulti[f], grid, dim3(256), 0, st, d_cs);
      for (int q = nj - 1; q >= 0; --q) record(cs[q]);
    });
    return outs;
  }

  // An edge of the layer graph on the tape: y = A src (or A^T src) now, src.g += the adjoint of y.g on the way back.
  void conv(const TConv& a, const TT& src, const TT& y) {
    hipLaunchKernelGGL(k_tconv, dim3((unsigned)((y.n + 3) / 4)), dim3(256), 0, st, a);
    TConv b = a;
    b.src = y.g; b.dst = src.g; b.dir = 1 - a.dir; b.acc = 1;
    const long nsrc = src.n;
    tape.push_back([b, nsrc, st = st]() { hipLaunchKernelGGL(k_tconv, dim3((unsigned)((nsrc + 3) / 4)), dim3(256), 0, st, b); });
  }
  void dense(const TDense& a, const TT& src, const TT& y) {
    hipLaunchKernelGGL(k_tdense, dim3((unsigned)y.n), dim3(TD_WAVES * 64), 0, st, a);
    TDense b = a;
    b.src = y.g; b.dst = src.g; b.dir = 1 - a.dir; b.acc = 1;
    const long nsrc = src.n;
    tape.push_back([b, nsrc, st = st]() { hipLaunchKernelGGL(k_tdense, dim3((unsigned)nsrc), dim3(TD_WAVES * 64), 0, st, b); });
  }

  // the weight gradients of every recorded op: two launches behind the backward walk
  std::vector<int> h_first;
  int weight_grads() {
    const int nops = (int)wops.size();
    if (!nops) return 0;
    h_first.assign(nops + 1, 0);
    for (int o = 0; o < nops; ++o) h_first[o + 1] = h_first[o] + wops[o].nchunks;
    const size_t op_floats = (sizeof(TLin) * nops + 3) / 4, first_floats = nops + 1;
    TLin* d_ops = reinterpret_cast<TLin*>(arena.alloc(op_floats));
    int* d_first = reinterpret_cast<int*>(arena.alloc(first_floats));
    if (!d_ops || !d_first) return 1;
    if (table(d_ops, wops.data(), sizeof(TLin) * nops) || table(d_first, h_first.data(), sizeof(int) * (nops + 1))) return 1;
    hipLaunchKernelGGL(k_tlin_bwd_w_all, dim3((unsigned)h_first[nops], 3), dim3(256), 0, st, d_ops, d_first, nops);
    hipLaunchKernelGGL(k_tlin_reduce_all_wide, dim3((64 * 193 + 255) / 256, (unsigned)L_COUNT), dim3(256), 0, st, d_ops, nops);
    return 0;
  }
};

}  // namespace gnnb_train
