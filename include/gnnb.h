/*
 * gnnb.h -- C-ABI of libgnnb.so: the MI355X (gfx950) GNN branching-score forward pass.
 *
 * The reference (oval-group/GNN_branching) is pure Python/PyTorch and has NO native
 * interface for this path; the entry points below are what a binding for the hot path
 * would call.  Each one cites the reference code it replaces.  Plain pointers and sizes
 * only -- no torch types.  The Python host side (gnn_branching_amd/graphnet) binds them
 * with ctypes; INTEGRATION.md shows the stub a reference maintainer would add.
 *
 * Conventions: every function returns 0 on success or a negative GNNB_E_* code and never
 * throws; gnnb_last_error() returns a thread-local message for the last failure.
 * gnnb_forward is stream-ordered and asynchronous, allocates nothing and never
 * synchronises; one handle per host thread (no entry point is re-entrant on one handle).  No HIP
 * call happens at library load time (the reference creates its GPU context inside a forked child:
 * experiments/bab_mip.py:244-249).  The library reads NO environment variable: every switch is a
 * handle option (gnnb_set_option).
 */
#ifndef GNNB_H
#define GNNB_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GNNB_ABI_VERSION 2

enum {
  GNNB_OK = 0,
  GNNB_E_INVALID = -1,   /* bad argument / unsupported shape */
  GNNB_E_HIP = -2,       /* a HIP runtime call failed */
  GNNB_E_STATE = -3,     /* call order (e.g. forward before bind_network) */
  GNNB_E_NOMEM = -4      /* workspace too small */
};

/* layer kinds of the verified network's layer list (reference graph_conv.py:110,130,139,188
 * dispatches on type(layer) is nn.Conv2d / nn.Linear / nn.ReLU / Flatten) */
enum { GNNB_CONV = 0, GNNB_LINEAR = 1, GNNB_RELU = 2, GNNB_FLATTEN = 3 };

typedef struct gnnb_handle gnnb_t;

/* One entry of layers['fixed_layers'] (reference plnn/relu_conv_gnnkwthreshold.py:111-112).
 * weight/bias are HOST pointers in torch's row-major layout (conv: [c_out][c_in][kh][kw],
 * linear: [n_out][n_in]); they are copied, the caller keeps ownership. */
typedef struct {
  int32_t kind;
  int32_t c_in, c_out, kh, kw, stride, pad;   /* GNNB_CONV  (square stride/pad, dilation 1, groups 1) */
  int32_t n_in, n_out;                         /* GNNB_LINEAR */
  const float* weight;
  const float* bias;
} gnnb_layer_desc;

/* One batch of B subproblems = the tensor arguments of GraphNet.forward
 * (reference graph_conv.py:479) as DEVICE pointers to contiguous fp32 arrays.
 * The pointer tables themselves (lb, ub, dual, primal) are HOST arrays. */
typedef struct {
  const float* const* lb;      /* n_graph ptrs: lower_bounds_all[k], (B, N_k)                */
  const float* const* ub;      /* n_graph ptrs: upper_bounds_all[k]                          */
  const float* const* dual;    /* n_relu  ptrs: dual_vars[j], (B*N_{j+1}, 3)                 */
  const float* const* primal;  /* n_primal ptrs: primals[m], (B*n_m), one per net.layers[m]  */
  const float* x_lp;           /* primal_inputs (B, N_0)                                     */
  const float* prop_w;         /* layers['prop_layers'][b].weight, (B, N_L)                  */
  const float* prop_b;         /* layers['prop_layers'][b].bias,   (B)                       */
  const float* mask;           /* masks (B, R): 1.0 where the BaB mask is -1                 */
  int32_t n_graph, n_relu, n_primal;
} gnnb_batch;

/* GraphNet(T, p) + load_state_dict (reference graph_score.py:9-13, graph_conv.py:22-74,
 * :421-432): w_blob = the 52 tensors of the checkpoint concatenated in state-dict order
 * (weight (out,in) row-major, then bias), 117 825 floats for T=2, p=64.  HOST pointer. */
int gnnb_create(gnnb_t** out, const float* w_blob, size_t n_floats, int T, int p);

/* Handle options.  The reference has one implementation of the path and therefore no switches (graph_conv.py:77-388); here an option
 * selects between kernels that compute the same scores, which is what lets the parity tests check them against each other and lets a
 * caller that shares the GPU (two batches in flight, a collective on another stream) turn off what needs co-resident workgroups.
 * Set options after gnnb_create; the ones marked (*) shape the tables of gnnb_bind_network and return GNNB_E_STATE on a bound handle.
 *   "bf3"          1 (default): 64x64 node-MLP blocks on the bf16 matrix rate, both operands in three bf16 pieces, fp32 accumulate
 *                  (fp32-grade); 0: every block on the exact-fp32 MFMA (and the separate kernels instead of k_top)
 *   "fuse"         1: a conv half-pass (graph_conv.py:110-181, :299-349) is ONE kernel; 0: aggregate kernel + node-update kernel
 *   "top"          1: last Linear edge, last ReLU layer, property node (graph_conv.py:130-137, :194-210, :320-326) in k_top; 0: separate kernels
 *   "gather" (*)   1: conv edges as MFMA tap blocks; 0: the scalar conv kernels
 *   "embed_fuse"   1: round 0's input embedding (graph_conv.py:90-95) computed inside the first aggregate; 0: written by k_embed
 *   "dense_lds" (*) 1: Linear edges one workgroup per sample out of LDS; 0: the per-tile kernel (what very wide layers fall back to)
 *   "tail_max_b"   batches up to it run the last restricted update + score head (graph_conv.py:442-470) as ONE launch; 0: three kernels
 *   "top_split"    1 / 2 / 4: most workgroups k_top spreads one sample over.  2 and 4 make workgroups WAIT for partner workgroups and
 *                  need all of them resident: set 1 when anything else may occupy CUs while a forward runs (status bit 1 otherwise)
 *   "top_fuse_upd" 1: the backward update of layer L-1 (graph_conv.py:253-350) inside k_top; 0: its own launch
 *   "clspre_max_b" batches up to it classify nodes and run the hoisted feature chains in one launch
 * gnnb_option_count / gnnb_option_name enumerate the table; gnnb_get_option reads a value back. */
int gnnb_set_option(gnnb_t* h, const char* name, int value);
int gnnb_get_option(const gnnb_t* h, const char* name, int* value);
int gnnb_option_count(void);
const char* gnnb_option_name(int i);

/* The verified network's fixed layers, i.e. the static part of the `layers` argument
 * (reference relu_conv_gnnkwthreshold.py:110-113; graph structure walked at
 * graph_conv.py:107-192 and :222-385).  (c0,h0,w0) = input tensor shape. */
int gnnb_bind_network(gnnb_t* h, const gnnb_layer_desc* layers, int n_layers, int c0, int h0, int w0);

/* Sizes of the bound layer graph: n_graph = L+2 graph layers, sizes[k] = N_k, *n_relu_total = R. */
int gnnb_graph_info(const gnnb_t* h, int* n_graph, int* sizes /* >= n_graph ints or NULL */, int* n_relu_total);

/* Bytes of device scratch gnnb_forward needs for a batch of B (embeddings `mu`, init_mu
 * graph_conv.py:487-496, plus aggregation and cached feature terms). */
size_t gnnb_workspace_bytes(const gnnb_t* h, int B);

/* GraphNet.forward + the argmax of GraphChoice.decision (reference graph_conv.py:479-483,
 * graph_score.py:32-47).  scores_padded: device (B, R) fp32, score of every ambiguous ReLU in
 * flat ReLU order, -inf elsewhere (the reference returns the ragged list of graph_conv.py:470).
 * decisions: device (B, 2) int32 [dec_lay, dec_idx], first maximal score; [-1,-1] if a sample
 * has no ambiguous ReLU.  status: device int32[1], bit 0 set if an embedding was NaN (the reference
 * enters pdb, graph_conv.py:184-186, :339-341), bit 1 if a wait inside a kernel (k_gather_update_q's LDS ring; k_top's workgroup
 * split waiting for its partner workgroups -- option "top_split" = 1 turns that split off) hit its iteration cap (never in a correct run on a
 * GPU the caller does not share with long-running kernels; the results are then invalid).  stream: hipStream_t (NULL = default).
 * Limit: every pixel below an inner convolution (the edge into ReLU layer k >= 2) must be read by at least one of its windows.  A stride
 * larger than the kernel leaves pixels with a tap count of 0, by which the reference divides the transposed aggregate
 * (graph_conv.py:306-312: 0/0, it stops).  gnnb_forward, gnnb_forward_host and gnnb_online_step refuse such a network with
 * GNNB_E_INVALID before anything is launched, naming the layer; the handle stays usable.  The first convolution is not normalised
 * and may skip pixels; gnnb_bind_network, gnnb_kw_bounds and gnnb_babsr divide by no tap count and accept the network. */
int gnnb_forward(gnnb_t* h, const gnnb_batch* in, int B, float* scores_padded, int32_t* decisions,
                 int32_t* status, void* workspace, size_t workspace_bytes, void* stream);

/* gnnb_forward for HOST inputs -- the reference's own call pattern (relu_conv_gnnkwthreshold.py:117, :230, :239: one
 * subproblem per graph.decision call, every argument a CPU tensor that graph_score.py:26-30 moves with ~14 .cuda() calls).
 * `in` holds HOST pointers laid out exactly as for gnnb_forward.  The inputs cross PCIe as ONE pinned copy, the forward runs
 * on `stream`, and decisions (B, 2), status (1) and -- if scores is not NULL -- the padded scores (B, R) are written to HOST
 * memory; the call returns after synchronising `stream`.  Staging buffers and the workspace belong to the handle. */
int gnnb_forward_host(gnnb_t* h, const gnnb_batch* in, int B, float* scores, int32_t* decisions, int32_t* status, void* stream);

/* Host-fed batches, fewer bytes over the link (reference graph_score.py:26-30 moves EVERY tensor whole).  Of `dual_vars` and `primals` the
 * forward reads only the entries of AMBIGUOUS ReLU nodes (the relaxation terms of graph_conv.py:153-161 and :273-293 are multiplied by
 * amb = 0 everywhere else) and the network output primals[-1]: 4 floats for ~7 % of the nodes instead of 5 for all of them.
 *   gnnb_amb_records_bytes   upper bound of the record image of a batch of B (every node ambiguous)
 *   gnnb_pack_amb_records    HOST: `in` holds HOST pointers laid out as for gnnb_forward (only lb / ub of the ReLU layers, dual, primal
 *                            are read).  Writes to `dst` (host memory, e.g. pinned; >= cap bytes) for every ReLU layer the nodes with
 *                            lb < 0 < ub -- a superset of the nodes the device classifies as ambiguous -- as records {layer, flat index
 *                            b N_k + n, dual[:, 1], dual[:, 2], primal_pre, primal_post} in no particular order, then primals[-1];
 *                            *used = bytes written.  Runs on up to a dozen helper threads that belong to the handle (created on first
 *                            use under a lock in the handle, shared with gnnb_forward_host's staging, joined by gnnb_destroy); the
 *                            handle gives them one job at a time, so concurrent packs on one handle take turns.  Every tensor's
 *                            element count is the caller's responsibility (B N_k per bound / primal tensor, 3 B N_k per dual tensor
 *                            of the BOUND network); x_lp, prop_w, prop_b and mask are not read and may be NULL.
 *   gnnb_scatter_amb_records DEVICE: one launch on `stream` that writes the records of an image copied to device memory into full-size
 *                            device arrays dual[k] (B N_k, 3) / primal[m] laid out as gnnb_forward expects them; entries of other nodes
 *                            are left as they are (the forward never reads them).  Then call gnnb_forward on those arrays: scores are
 *                            the bits of a forward on the whole tensors.  status: device int32[1] the caller zeroed, or NULL; bit 2
 *                            (value 4) is set -- and nothing, or not that record, is written -- when the image's header does not match
 *                            this binding and B, or a record points outside its arrays (a stale or foreign image). */
size_t gnnb_amb_records_bytes(const gnnb_t* h, int B);
int gnnb_pack_amb_records(const gnnb_t* h, const gnnb_batch* in, int B, void* dst, size_t cap, size_t* used);
int gnnb_scatter_amb_records(gnnb_t* h, const void* dev_image, int B, float* const* dual, int n_relu, float* const* primal, int n_primal,
                             int32_t* status, void* stream);

/* BaBSR ("KW") branching heuristic for a batch -- the fallback scorer of the BaB loop (reference
 * plnn/kw_score_conv.py choose_node_conv :41-113, called at plnn/relu_conv_gnnkwthreshold.py:157).  lb/ub: HOST tables of
 * n_graph DEVICE pointers laid out like struct gnnb_batch.lb, .ub -- only the ReLU layers 1..L are read; prop_w (B, N_L); mask (B, R) 1.0 where the
 * BaB mask is -1.  Outputs, device (B, R): scores = `score` (:103), intercepts = `intercept_tb` (:86), both already
 * multiplied by the mask; a 0/0 slope's NaN propagates as in torch.  The decision rule (:115-156, with its counters and random
 * fall-back) stays on the host.  GNNB_E_INVALID before any launch when the widest ReLU layer has more than 20480 nodes (its two fp32
 * ratio buffers would need more than 160 KiB of LDS). */
int gnnb_babsr(gnnb_t* h, const float* const* lb, const float* const* ub, int n_graph, const float* prop_w,
               const float* mask, int B, float* scores, float* intercepts, void* stream);

/* Wong-Kolter intermediate bounds of B BaB domains, fp64 (reference plnn/dual_network_linear_approximation.py init_kw_bounds :205-294 and
 * update_kw_bounds :296-451 on the dual network of convex_adversarial/dual_network.py:15-121; restated on the host by
 * gnn_branching_amd/lp_producer.py LayerGraphLP.kw_bounds).  Per affine layer, in order: the interval image of the bounds below; from
 * the second affine layer on, the KW bound of every output node (one dual-network backward pass per node, reading the mask-clamped
 * bounds of the ReLUs below) intersected with it; the parent's bounds intersected; the split mask applied to the pre-activation
 * bounds (1: lo >= 0, 0: up <= 0).  A domain with a parent (split_layer[b] >= 0) keeps the parent's bounds of graph layers
 * 1..split_layer[b]+1 bit for bit (then the mask), the layers above are recomputed and intersected with the parent's.  The last
 * affine layer is the domain's property layer.  A domain's bounds do not depend on B or on its place in the batch.
 * All pointers inside the struct are DEVICE pointers; the pointer tables parent_lb / parent_ub are HOST arrays. */
typedef struct {
  const double* x_lo;                 /* input box (B, N_0), one per domain                                         */
  const double* x_hi;
  const float* prop_w;                /* property layers as in gnnb_batch: (B, N_L) and (B)                          */
  const float* prop_b;
  const int8_t* mask;                 /* BaB mask (B, R) in flat ReLU order: -1 undecided, 0 blocked, 1 passing     */
  const double* const* parent_lb;     /* NULL, or n_graph-1 ptrs: the parents' bounds of graph layers 1..L+1 (B, N_k) */
  const double* const* parent_ub;
  const int32_t* split_layer;         /* (B): ReLU layer (0..L-1) of the split that made the domain, -1 (any negative
                                         value) = no parent; values >= L count as L-1.  Required with parent_lb      */
  int32_t n_graph;                    /* L + 2, as gnnb_graph_info reports                                          */
} gnnb_kw_batch;

/* Bytes of device workspace gnnb_kw_bounds needs for a batch of B (0 for a null or unbound handle). */
size_t gnnb_kw_workspace_bytes(const gnnb_t* h, int B);

/* lb / ub: HOST tables of n_graph-1 DEVICE pointers, graph layers 1..L+1, (B, N_k) fp64, mask applied.  lb32 / ub32: NULL, or n_graph
 * pointers laid out as gnnb_batch.lb / .ub (layer 0 = the box), the same bounds rounded to fp32: they feed gnnb_babsr and gnnb_forward
 * directly.  infeasible: device (B) int32, 1 where some lo > up + 1e-9 (the test LayerGraphLP.solve applies).  Stream-ordered, no
 * allocation, no synchronisation; the workspace needs no initialisation.  GNNB_E_INVALID for a null handle or a network whose widest
 * ReLU layer exceeds 4096 nodes (the dual pass holds two of them in LDS). */
int gnnb_kw_bounds(gnnb_t* h, const gnnb_kw_batch* in, int B, double* const* lb, double* const* ub, float* const* lb32, float* const* ub32,
                   int32_t* infeasible, void* workspace, size_t workspace_bytes, void* stream);

/* gnnb_kw_bounds with the bounds of every ambiguous node (mask -1, l < 0 < u) of graph layers 2..L tightened by dual ascent, fp64
 * (restated on the host by LayerGraphLP.kw_bounds(tighten=n)).  Layers go in order.  Behind the Wong-Kolter pass
 * of a layer, its bounds are met with gnnb_kw_bounds' own (computed first, into the workspace), then every node that is still ambiguous
 * runs, for its lower and for its upper bound, n_iter steps of gnnb_dual_ascent's recursion (projected Adam, step lr, n_iter + 1
 * evaluations, the best kept; start alpha = u / (u - l), beta = 0) on the network cut off below the layer with +e_j / -e_j in place of
 * the property row; beta is free on the split nodes of the node's receptive field.  The layer's mask, relaxation and fp32 copies are
 * then redone from the tightened bounds before the layer above reads them.  Layers a child copies from its parent are not touched; layer
 * 1 is exact and the property layer is gnnb_dual_ascent's.  No bound is looser than gnnb_kw_bounds'; n_iter = 0 launches what
 * gnnb_kw_bounds launches and equals it bit for bit.  A domain's bounds do not depend on B or on its place in the batch. */

/* Bytes of device workspace gnnb_kw_tighten needs for a batch of B besides gnnb_kw_bounds' (0 for a null or unbound handle): per
 * domain R flag bytes, 2 R + 2 (N_1 + .. + N_L + 1) doubles of the plain chain, and for the layers whose per-node state (7 n + n_0
 * doubles, n / n_0: the nodes / inputs of the node's receptive field) does not fit in LDS behind the two lambda buffers, the largest
 * N_k (7 n + n_0). */
size_t gnnb_kw_tighten_workspace_bytes(const gnnb_t* h, int B);

/* in, lb, ub, lb32, ub32, infeasible, kw_workspace: gnnb_kw_bounds' arguments, with its checks.  counts: NULL, or device (B, 2) int32:
 * per domain the nodes the ascent ran for and how many of them it decided (no longer l < 0 < u).  Stream-ordered, no allocation, no
 * synchronisation; the workspaces need no initialisation.  Refused before any launch: GNNB_E_INVALID for a null handle or argument,
 * B < 1, n_iter < 0, lr not a positive finite number or a network whose widest ReLU layer exceeds 4096 nodes; GNNB_E_STATE before
 * gnnb_bind_network; GNNB_E_NOMEM for a short workspace. */
int gnnb_kw_tighten(gnnb_t* h, const gnnb_kw_batch* in, int B, int n_iter, double lr, double* const* lb, double* const* ub,
                    float* const* lb32, float* const* ub32, int32_t* infeasible, int32_t* counts, void* kw_workspace,
                    size_t kw_workspace_bytes, void* workspace, size_t workspace_bytes, void* stream);

/* Lower bounds of B BaB domains by dual ascent on their LP relaxation, fp64 -- stands in for the LP the reference builds and solves
 * with Gurobi (plnn/conv_kwinter_gen.py:179-555: build_the_model, its optimum and the primal / dual point GraphChoice.decision reads)
 * wherever the optimum is wanted to a few digits; restated on the host by gnn_branching_amd/lp_producer.py LayerGraphLP.dual_value /
 * dual_ascent_host / dual_recover.  With the intermediate bounds of gnnb_kw_bounds fixed, the LP's dual is the
 * Wong-Kolter dual network with a free slope alpha in [0, 1] on the lower relaxation of every ambiguous ReLU (mask -1, l < 0 < u) and
 * one multiplier beta >= 0 per split node (mask 0 / 1).  Every (alpha, beta) gives a sound lower bound g on the property output; the
 * maximum is the LP optimum.  One workgroup per domain runs n_iter steps of projected Adam (ascent; b1 0.9, b2 0.999, eps 1e-8, step
 * lr) on the exact supergradient, n_iter + 1 evaluations of g, and keeps the best.  A domain's result does not depend on B or on its
 * place in the batch.
 * All pointers inside the struct are DEVICE pointers; the tables lb / ub are HOST arrays of n_graph-1 device pointers. */
typedef struct {
  const double* const* lb;            /* graph layers 1..L+1 (B, N_k) as gnnb_kw_bounds writes them (mask applied); layer L+1 is not read */
  const double* const* ub;
  const double* x_lo;                 /* input box (B, N_0)                                                          */
  const double* x_hi;
  const float* prop_w;                /* property layers as in gnnb_batch: (B, N_L) and (B)                          */
  const float* prop_b;
  const int8_t* mask;                 /* BaB mask (B, R) in flat ReLU order: -1 undecided, 0 blocked, 1 passing     */
  int32_t n_graph;                    /* L + 2                                                                       */
} gnnb_dual_batch;

/* Bytes of device workspace gnnb_dual_ascent needs for a batch of B (0 for a null or unbound handle). */
size_t gnnb_dual_workspace_bytes(const gnnb_t* h, int B);

/* alpha / beta: device (B, R) fp64, flat ReLU order, in and out.  warm = 0: the start is alpha = u / (u - l), beta = 0 (g there is the
 * property-layer lower bound gnnb_kw_bounds computes before its interval intersection); warm = 1: the start is what the arrays hold
 * (a child starts from its parent's point), projected onto alpha in [0, 1], beta >= 0, beta = 0 on unsplit nodes.  On return they hold
 * the best point met and bound (B) its value g; n_iter = 0 evaluates g at the start.  alpha of a node that is not ambiguous is ignored.
 * grad_alpha / grad_beta: both NULL, or (B, R): the supergradient at the start (inspection, tests).
 * dual / primal / x_lp: all NULL, or the scorer's inputs at the best point, fp32, laid out as gnnb_batch's (dual: n_relu pointers (B N_k, 3);
 * primal: n_primal pointers, of which the pre- and post-activation of every ReLU layer and primals[-1] must be given and are written,
 * any other entry may be NULL; x_lp (B, N_0)): the minimiser x* of the inner problem, the pre-activations and the ReLU ENVELOPE values of
 * the forward pass from it (max(pre, 0) where the node's dual coefficient lambda >= 0, s pre + t where lambda < 0), the property output
 * there, and dual[:, 0] = 0, dual[:, 1] = alpha max(lambda, 0) >= 0 (Pi of v >= pre), dual[:, 2] = min(lambda, 0) <= 0 (Pi of
 * v <= s pre + t), zero on decided nodes -- the sign convention of the reference's Pi.  gnnb_forward reads them without a host round trip.
 * lb32_prop: NULL, or (B) fp32: the bound, e.g. the property entry of gnnb_kw_bounds' lb32 table (where the reference puts the LP optimum).
 * Stream-ordered, no allocation, no synchronisation; the workspace needs no initialisation.  GNNB_E_INVALID for a null handle, B < 1,
 * n_iter < 0 or a network whose widest ReLU layer exceeds 4096 nodes (refused before a launch: two fp64 buffers of it live in LDS);
 * GNNB_E_NOMEM for a short workspace; GNNB_E_STATE before gnnb_bind_network. */
int gnnb_dual_ascent(gnnb_t* h, const gnnb_dual_batch* in, int B, int n_iter, double lr, double* alpha, double* beta, int warm,
                     double* bound, double* grad_alpha, double* grad_beta, float* const* dual, float* const* primal, float* x_lp,
                     float* lb32_prop, void* workspace, size_t workspace_bytes, void* stream);

/* ---- a branch-and-bound frontier in device memory (gnn_branching_amd/frontier.py runs the loop) ----
 * The steps of one BaB round (reference plnn/relu_conv_gnnkwthreshold.py:126-262: pick a domain, split it, bound the children, keep or
 * close them) that the batch entry points above do not cover, for K domains at once, reading and writing DEVICE arrays only.  A round:
 * frontier_gather -> dual_ascent (n_iter 0, warm 1, scorer inputs) -> forward -> frontier_expand -> kw_bounds -> dual_ascent ->
 * net_eval -> frontier_commit, then one copy of the state record to the host.  All of them are stream-ordered, allocate nothing and never
 * synchronise; GNNB_E_INVALID for a null handle or argument, K < 1 (K > 32767) or a network whose widest ReLU layer exceeds 4096 nodes
 * (the cap of the kernels they run between), GNNB_E_STATE before gnnb_bind_network, GNNB_E_NOMEM for a short workspace -- all before any
 * launch.  No kernel waits on another workgroup; every minimum and count is a fixed tree in a fixed order.
 *
 * The POOL: `capacity` slots the caller owns, a struct of device arrays.  lb / ub are HOST tables of n_graph-1 device pointers. */
typedef struct {
  int8_t* mask;                       /* (capacity, R) BaB masks, resolved by the bounds                               */
  double* const* lb;                  /* graph layers 1..L+1 (capacity, N_k), mask applied, as gnnb_kw_bounds writes them */
  double* const* ub;
  double* alpha;                      /* (capacity, R) the dual point `bound` belongs to (gnnb_dual_ascent's best)     */
  double* beta;
  double* bound;                      /* (capacity) lower bound of the domain                                          */
  int32_t* open;                      /* (capacity) 1: the slot holds an open domain.  The caller zeroes it once       */
  int32_t capacity, n_graph;
} gnnb_pool;

/* The 2K children of a round as the batch entry points left them (row 2i: parent i with the decided node blocked, 2i+1: passing). */
typedef struct {
  const int8_t* mask;                 /* (2K, R) as gnnb_frontier_expand wrote it                                      */
  const double* const* lb;            /* gnnb_kw_bounds' outputs, HOST tables of n_graph-1 device pointers (2K, N_k)   */
  const double* const* ub;
  const int32_t* infeasible;          /* (2K) gnnb_kw_bounds                                                           */
  const double* bound;                /* (2K) gnnb_dual_ascent                                                         */
  const double* alpha;                /* (2K, R)                                                                       */
  const double* beta;
  const double* ub_value;             /* (2K) gnnb_net_eval at gnnb_dual_ascent's x_lp                                 */
  const int32_t* live;                /* (2K) gnnb_frontier_expand                                                     */
  int32_t n_graph;
} gnnb_children;

/* The state record: GNNB_FRONTIER_STATE_DOUBLES device doubles (counts are whole numbers): [0] global_ub, [1] closed_lb (lowest bound
 * of a closed leaf), [2] lowest open bound (+inf: none), [3] open domains, [4] slots in use (1 + the highest slot ever written),
 * [5] / [6] / [7] children kept / closed / infeasible in the last commit, [8] kept children that found no slot (closed at their bound
 * instead, which keeps closed_lb sound; never with slots_in_use + 2K <= capacity).  Start: {+inf, +inf, +inf, 0, 0, ...}. */
#define GNNB_FRONTIER_STATE_DOUBLES 9

/* slots: device (K) int32, distinct slots of the pool.  x_lo / x_hi: device (K, N_0), the box of every row.  Writes row i of: mask (K, R);
 * lb / ub (HOST tables of n_graph-1 device pointers, (K, N_k) fp64); lb32 / ub32 (n_graph pointers laid out as gnnb_batch.lb / .ub: layer 0
 * the box, the others the pool's bounds rounded to nearest, as gnnb_kw_bounds' lb32); alpha / beta (K, R); scorer_mask (K, R) fp32, 1.0
 * where the mask is -1 (gnnb_batch.mask).  gnnb_dual_ascent with n_iter = 0, warm = 1 on these rows re-derives the scorer's inputs. */
int gnnb_frontier_gather(gnnb_t* h, const gnnb_pool* pool, const int32_t* slots, int K, const double* x_lo, const double* x_hi, int8_t* mask,
                         double* const* lb, double* const* ub, float* const* lb32, float* const* ub32, double* alpha, double* beta,
                         float* scorer_mask, void* stream);

/* decisions: device (K, 2) int32 as gnnb_forward writes them.  Writes rows 2i (blocked) and 2i+1 (passing) of: mask (2K, R), the parent's
 * with the decided node set to 0 / 1; parent_lb / parent_ub (HOST tables of n_graph-1 device pointers (2K, N_k)) and split_layer (2K):
 * gnnb_kw_batch's; alpha / beta (2K, R): the parent's point, the warm start; live (2K) int32.  A parent whose decision is [-1, -1]
 * (or names no node) yields two rows with live = 0, the parent's mask and split_layer = L-1: complete rows the batch entry points can
 * run on, which gnnb_frontier_commit ignores. */
int gnnb_frontier_expand(gnnb_t* h, const gnnb_pool* pool, const int32_t* slots, const int32_t* decisions, int K, int8_t* mask,
                         double* const* parent_lb, double* const* parent_ub, int32_t* split_layer, double* alpha, double* beta, int32_t* live,
                         void* stream);

/* The bound network followed by row b of the property layers at B points, fp64 (the upper bound the BaB loop takes from a forward pass at
 * the LP's input point, reference plnn/conv_kwinter_gen.py:514-519).  x: device (B, N_0) fp32 as gnnb_dual_ascent writes x_lp; prop_w
 * (B, N_L), prop_b (B) as in gnnb_batch; out: device (B) fp64.  A point's value does not depend on B or on its row. */
size_t gnnb_net_eval_workspace_bytes(const gnnb_t* h, int B);
int gnnb_net_eval(gnnb_t* h, const float* x, const float* prop_w, const float* prop_b, int B, double* out, void* workspace,
                  size_t workspace_bytes, void* stream);

/* ---- the second half of the reference's upper bound: descent on the real network from the LP point ----
 * Projected signed-gradient descent on f(x) = gnnb_net_eval's value at the fp32 point x, per point, fp64: what get_upper_bound_pgd
 * (reference plnn/conv_kwinter_gen.py:54-135) does from each child's LP point once the incumbent is positive
 * (plnn/relu_conv_any_kw.py:143-149).  g(x) is the backward pass through the activations of f's own forward pass: g_L = prop_w where the
 * last ReLU layer is positive, down every edge by its transpose, gated by 1[activation > 0] at every ReLU layer (torch's ReLU gradient),
 * every sum in a fixed order.  The rule, per point: best = (f(x0), x0), unconditionally; for t = 0 .. n_steps - 1
 *   x_{t+1}[m] = fl32(min(max((double)x_t[m] - step (x_hi[m] - x_lo[m]) sgn(g_t[m]), x_lo[m]), x_hi[m])),  sgn(0) = 0,
 * rounded to nearest and, where rounding leaves [x_lo, x_hi], moved to the neighbouring float inside; f(x_{t+1}) < best, strictly, makes
 * it the best; if not f(x_{t+1}) < f(x_t) the point stops (the reference's stop rule, :110; no comparison holds for a NaN).  A point with
 * a NaN coordinate in x0, or whose f(x0) is NaN, takes no step.  Deliberately NOT the reference's: its 2056 random restarts (they are
 * gnnb_net_starts / gnnb_net_descend_starts below) and its step size, a min over the whole batch (:113-122), which would make a row depend on its
 * batch.
 * x0: device (B, N_0) fp32; x_lo / x_hi: device (B, N_0) fp64; prop_w (B, N_L), prop_b (B) fp32 as in gnnb_net_eval; step in (0, 1]: the
 * share of the box's width a coordinate moves per step.  Outputs, device: x_best (B, N_0) fp32 (must not overlap x0); value (B) fp64 =
 * f(x_best), bit for bit gnnb_net_eval's; grad0: NULL, or (B, N_0) fp64, g(x0), for inspection; steps_taken: NULL, or (B) int32, the
 * steps evaluated.  n_steps = 0 gives x_best = x0 and value = gnnb_net_eval(x0), bit for bit.  One workgroup per point; the workspace
 * holds the activations of every graph layer 0..L and two gradient buffers of the widest layer per point.  Stream-ordered, no allocation,
 * no synchronisation, no atomics, no workgroup waits on another; a point's result does not depend on B or on its row.  GNNB_E_INVALID
 * before any launch for a null handle or argument, B < 1, n_steps < 0 or a step outside (0, 1]; GNNB_E_STATE before gnnb_bind_network;
 * GNNB_E_NOMEM for a short workspace. */
size_t gnnb_net_descend_workspace_bytes(const gnnb_t* h, int B);
int gnnb_net_descend(gnnb_t* h, const float* x0, const double* x_lo, const double* x_hi, const float* prop_w, const float* prop_b, int B,
                     int n_steps, double step, float* x_best, double* value, double* grad0, int32_t* steps_taken, void* workspace,
                     size_t workspace_bytes, void* stream);

/* ---- the upper bound from many starts: get_upper_bound_pgd's restarts (reference plnn/conv_kwinter_gen.py:54-135:
 * the LP point in slot 0, uniform points of the domain in the others) and get_upper_bound_random (:20-52) on the device ----
 * gnnb_net_starts writes the start points of B rows.  x0: device (B, N_0) fp32; x_lo / x_hi: device (B, N_0) fp64; starts: device
 * (B, R + 1, N_0) fp32 (must not overlap x0); R in 0..4096 random starts per row; seed: any 64 bits.  Slot 0 of row b is x0[b], bit for
 * bit.  Slot r >= 1 is a counter-based uniform point of the row's box, with all integer arithmetic mod 2^64:
 *   G = 0x9E3779B97F4A7C15;  mix(z): z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9; z = (z ^ (z >> 27)) * 0x94D049BB133111EB; z ^ (z >> 31)
 *   key_b = seed + sum_m mix(bits32(x0[b, m]) + (m << 32))          u(b, r, m) = (mix(key_b + G (r N_0 + m + 1)) >> 11) 2^-53, in [0, 1)
 *   value = fma(x_hi - x_lo, u, x_lo) in fp64, rounded to the nearest fp32, moved to the neighbouring float inside [x_lo, x_hi] where that
 *   rounding left it (gnnb_net_descend's move).
 * No generator state, no atomics: a row's starts depend on its own x0, box and seed only -- not on B, on its index or on what ran before.
 * A NaN in x0 stays in slot 0 (it reaches the other slots through the key only, by its bits).
 *
 * gnnb_net_descend_starts runs gnnb_net_descend's rule, unchanged, from every one of the n_starts (1..4097) start points of every row --
 * starts: device (B, n_starts, N_0) fp32, all of row b inside row b's box [x_lo[b], x_hi[b]] under row b's property row -- and picks per
 * row the minimum of the starts' best values in the total order (value, start index): strict <, in start order, a NaN never wins, the
 * first of equal values wins, and where every value is a NaN the result is start 0 and its NaN.  One workgroup carries
 * gnnb_net_descend_starts_tile() starts of one row through every layer together; start r of row b ends, bit for bit, where
 * gnnb_net_descend ends on that point as a row of its own, and value[b] is gnnb_net_eval(x_best[b]) bit for bit.  The one exception: a
 * start with a NaN coordinate takes no step, as there, but its value is a NaN (a ReLU swallows the NaN, and what gnnb_net_descend reports for
 * such a point is the network's value at no point of the box), so it never wins.  Outputs, device: x_best
 * (B, N_0) fp32 (must not overlap starts), value (B) fp64: the winner's; start_index: NULL, or (B) int32, the winner's slot; start_value:
 * NULL, or (B, n_starts) fp64, every start's best value; start_steps: NULL, or (B, n_starts) int32, every start's steps evaluated.
 * Both are stream-ordered, allocate nothing, never synchronise, use no atomics, and no workgroup waits on another.  GNNB_E_INVALID before
 * any launch for a null handle or required argument, B < 1, R outside 0..4096, n_starts outside 1..4097, n_steps < 0, a step outside
 * (0, 1] or an overlapping output; GNNB_E_STATE before gnnb_bind_network; GNNB_E_NOMEM for a short workspace. */
int gnnb_net_starts(gnnb_t* h, const float* x0, const double* x_lo, const double* x_hi, int B, int R, uint64_t seed, float* starts,
                    void* stream);
int gnnb_net_descend_starts_tile(void);
size_t gnnb_net_descend_starts_workspace_bytes(const gnnb_t* h, int B, int n_starts);
int gnnb_net_descend_starts(gnnb_t* h, const float* starts, int n_starts, const double* x_lo, const double* x_hi, const float* prop_w,
                            const float* prop_b, int B, int n_steps, double step, float* x_best, double* value, int32_t* start_index,
                            double* start_value, int32_t* start_steps, void* workspace, size_t workspace_bytes, void* stream);

/* Closes a round.  slots: the K parents (as given to gnnb_frontier_expand); eps; decision_bound (NaN: none); state: the record above,
 * read and updated.  In order: every live child's mask is resolved by its bounds (-1 with lo >= 0 -> 1, -1 with up <= 0 -> 0);
 * global_ub = min(global_ub, ub_value of every live feasible child); a live feasible child with an undecided node, bound <
 * global_ub - eps and (with a decision bound) bound < decision_bound is KEPT, every other live feasible child lowers closed_lb; a parent
 * without a live child lowers closed_lb by its own bound; the parents' slots are freed; the kept child of rank r (among the kept, in
 * child order) is stored in slot slots[r], from r = K on in slot in_use + (r - K) (in_use: state[4] before the call); the record is
 * updated.  The root enters a pool the same way: K = 1, slots = {0}, the root as child row 0 and live = {1, 0}. */
size_t gnnb_frontier_commit_workspace_bytes(const gnnb_t* h, int K);
int gnnb_frontier_commit(gnnb_t* h, const gnnb_pool* pool, const int32_t* slots, int K, const gnnb_children* children, double eps,
                         double decision_bound, double* state, void* workspace, size_t workspace_bytes, void* stream);

/* ---- several ReLUs per parent while a round is underfilled (frontier.py split_depth) ----
 * A round of K parents at DEPTH d (1..8) gives every parent C = 2^d child rows, [C i, C i + C), so that few parents still fill the child
 * side's rows; K << d is at most 65534.  Everything between the two calls (gnnb_kw_bounds, gnnb_dual_ascent, gnnb_net_eval, ...) runs on
 * the K << d rows unchanged.
 *
 * gnnb_frontier_expand_depth.  cand0: device (K + 1) int32 and cand_dec: device (n, 2) int32 as gnnb_strong_list writes them (n =
 * cand0[K]; parent i's nodes are entries [cand0[i], cand0[i+1]) in ascending flat index) -- with scores = gnnb_forward's scores_padded and
 * top_m = d the d undecided nodes the scorer ranks first, the first of them gnnb_forward's own decision.  With m_i = cand0[i+1] -
 * cand0[i], row C i + j is LIVE for j < 2^m_i: mask = the parent's with the b-th listed node (b = 0..m_i-1) set to bit b of j (0 blocked,
 * 1 passing); split_layer = the lowest layer among the m_i nodes; alpha / beta and the parent_lb / parent_ub rows = the parent's.  Every
 * other row of a parent in the pool is DEAD -- rows j >= 2^m_i, and all C rows when m_i = 0, m_i > d, the entries leave [0, n) or one of
 * them names no node of the network: the parent's mask, split_layer = L-1, live = 0, complete rows the batch entry points can run on.  A
 * slot outside the pool yields gnnb_frontier_expand's unread rows: live = 0, split_layer = -1, nothing else written.  At d = 1 with cand0
 * = {0, 1, .., K} and cand_dec = decisions every output is gnnb_frontier_expand's, bit for bit.  The other arguments are
 * gnnb_frontier_expand's, with K << d rows.
 *
 * gnnb_frontier_commit_depth.  gnnb_frontier_commit's rule on the (K << d) child rows: every live child is resolved and kept or closed
 * as there; a parent none of whose C rows is live lowers closed_lb by its own bound; ranks run in child order over all rows, the kept
 * child of rank r goes to slots[r] for r < K and to in_use + (r - K) from there on, so a round needs in_use + (C - 1) K <= capacity to
 * lose no child (state[8] counts the ones that found no slot; they are closed at their bound).  At d = 1 it is gnnb_frontier_commit, bit
 * for bit.  children: K << d rows.
 *
 * Both: stream-ordered, no allocation, no synchronisation, no atomics, no workgroup waits on another.  GNNB_E_INVALID before any launch
 * for a null handle or argument, K outside 1..32767, depth outside 1..8, K << depth above 65534 or a network past the 4096-node cap;
 * GNNB_E_STATE before gnnb_bind_network; GNNB_E_NOMEM for a short workspace (gnnb_frontier_commit_depth_workspace_bytes; 0 for a null or
 * unbound handle or sizes that would be refused). */
int gnnb_frontier_expand_depth(gnnb_t* h, const gnnb_pool* pool, const int32_t* slots, int K, int depth, const int32_t* cand0,
                               const int32_t* cand_dec, int8_t* mask, double* const* parent_lb, double* const* parent_ub,
                               int32_t* split_layer, double* alpha, double* beta, int32_t* live, void* stream);
size_t gnnb_frontier_commit_depth_workspace_bytes(const gnnb_t* h, int K, int depth);
int gnnb_frontier_commit_depth(gnnb_t* h, const gnnb_pool* pool, const int32_t* slots, int K, int depth, const gnnb_children* children,
                               double eps, double decision_bound, double* state, void* workspace, size_t workspace_bytes, void* stream);

/* ---- many jobs in one pool (gnn_branching_amd/frontier.py verify_properties runs the loop) ----
 * A JOB is a box, a property row and a decision bound on the bound network.  The pool is `segments` segments of `seg_cap` slots (segment
 * s: slots [s seg_cap, (s+1) seg_cap)), gnnb_pool.capacity = segments * seg_cap; a segment holds one job at a time and has its own state
 * record, so `state` is (segments, GNNB_FRONTIER_STATE_DOUBLES) and slots-in-use counts from the segment's first slot.  Inside its
 * segment a job runs the rule above with capacity = seg_cap, whatever else is in flight.
 *
 * A round's PLAN: n_entries entries {segment, row0, k} of int32, one per job that takes part, row0 the running sum of k, n the sum.
 * The job's k parents are rows [row0, row0 + k) of every (n, .) array, its children rows [2 row0, 2 row0 + 2k) of every (2n, .) array;
 * between the three entry points below run gnnb_frontier_gather / _expand (K = n) and the batch entry points (B = n or 2n) on global slot
 * numbers.  The entry points read `host` for their checks (before any launch), the kernels read `device`, which holds the same values.
 * Refused with GNNB_E_INVALID: a null handle or argument; no entry, n < 1 or n > 32767; an entry whose segment lies outside the pool or
 * whose k < 1; entries that do not tile the rows [0, n) in order; a pool whose capacity is not segments * seg_cap; a network past the
 * 4096-node cap.  GNNB_E_STATE before gnnb_bind_network, GNNB_E_NOMEM for a short workspace.  Stream-ordered, no allocation, no
 * synchronisation; no kernel waits on another workgroup, no reduction mixes two entries: an entry's result depends on its segment alone. */
typedef struct {
  const int32_t* host;                /* (n_entries, 3) {segment, row0, k}                                             */
  const int32_t* device;              /* the same values in device memory                                              */
  int32_t n_entries, n;
  int32_t segments, seg_cap;
} gnnb_plan;

/* Per entry: the k slots of lowest key among the segment's first slots-in-use, ascending, the key being the bound of an open slot and
 * +inf of a closed one, equal keys by slot.  Writes slots[row0 + r] (GLOBAL slot numbers) and row_seg[row0 + r] = segment; device (n). */
int gnnb_frontier_pick_jobs(gnnb_t* h, const gnnb_pool* pool, const gnnb_plan* plan, const double* state, int32_t* slots, int32_t* row_seg,
                            void* stream);

/* The rows the batch entry points read, from per-segment tables seg_x_lo / seg_x_hi (segments, N_0) fp64, seg_prop_w (segments, N_L),
 * seg_prop_b (segments) fp32: parent row i (x_lo / x_hi (n, N_0), prop_w (n, N_L), prop_b (n)) gets segment row_seg[i], child row c
 * (child_* with 2n rows) segment row_seg[c >> 1].  row_seg: device (n), as gnnb_frontier_pick_jobs wrote it. */
int gnnb_frontier_rows_jobs(gnnb_t* h, const gnnb_plan* plan, const int32_t* row_seg, const double* seg_x_lo, const double* seg_x_hi,
                            const float* seg_prop_w, const float* seg_prop_b, double* x_lo, double* x_hi, float* prop_w, float* prop_b,
                            double* child_x_lo, double* child_x_hi, float* child_prop_w, float* child_prop_b, void* stream);

/* gnnb_frontier_commit per entry: its children, its parents' slots (slots: device (n), global numbers), its segment (a kept child beyond
 * the segment's end is closed at its bound and counted in record [8]), its record, its decision bound (decision_bound: device
 * (segments) fp64, NaN: none).  children: the 2n rows.  Segments without an entry are not touched. */
size_t gnnb_frontier_commit_jobs_workspace_bytes(const gnnb_t* h, int n);
int gnnb_frontier_commit_jobs(gnnb_t* h, const gnnb_pool* pool, const gnnb_plan* plan, const int32_t* slots, const gnnb_children* children,
                              double eps, const double* decision_bound, double* state, void* workspace, size_t workspace_bytes, void* stream);

/* ---- the BaBSR fall-back below a branching threshold, inside a round ----
 * The control flow of reference plnn/relu_conv_gnnkwthreshold.py:151-195 for the K parents of a round, between the bounding of the GNN
 * decisions' children (pair A) and gnnb_frontier_commit: the improvement test (:151, :155), the BaBSR decision rule
 * (plnn/kw_score_conv.py:115-156, on gnnb_babsr's scores and intercepts of the parent rows), the skip of a point that was inefficient
 * kwbd_threshold times (:160-167) and, once the selected parents' second pair of children (pair B) is bounded, the choice between the two
 * pairs (:176-192).  The run's intercept counter and the table of inefficient points are read and updated in parent row order.
 * Both entry points are stream-ordered, allocate nothing and never synchronise; no atomics, no kernel waits on another workgroup, every
 * arg-max / arg-min is a fixed tree on the total order (value, index).  GNNB_E_INVALID for a null handle or argument, K < 1 (K > 32767),
 * m > K, thresholds outside their ranges or a network past the 4096-node cap, GNNB_E_STATE before gnnb_bind_network, GNNB_E_NOMEM for a
 * short workspace -- all before any launch. */
typedef struct {
  const int32_t* live;                /* (2K) pair A: gnnb_frontier_expand on the GNN's decisions                       */
  const int32_t* infeasible;          /* (2K) gnnb_kw_bounds                                                            */
  const double* bound;                /* (2K) gnnb_dual_ascent                                                          */
  const float* scores;                /* (K, R) gnnb_babsr on the parent rows gnnb_frontier_gather wrote                */
  const float* intercepts;            /* (K, R)                                                                         */
  const float* scorer_mask;           /* (K, R) gnnb_frontier_gather's: non-zero where the node is undecided            */
  double branching_threshold;         /* 0 < . <= 1: a parent whose GNN improvement is below it asks BaBSR (:155)       */
  double decision_threshold;          /* kw_score_conv.py:41 (0.001)                                                    */
  int32_t kwbd_threshold;             /* >= 0: a node counted inefficient this often is not bounded again (:160)        */
  int32_t sparsest_layer;
  const int32_t* random_order;        /* HOST (n_order): ReLU layers, popped from the end (relu_conv_gnnkwthreshold.py:97-103) */
  int32_t n_order;                    /* 0..8                                                                           */
  int32_t* icp;                       /* device (1) ((segments) in the jobs form): the intercept counter (:119), read and updated */
  const int32_t* ineff;               /* device (R) ((segments, R) in the jobs form): how often a node's KW split was inefficient */
} gnnb_fallback;

/* Per parent row i with a live pair A: gnn_improvement[i] = (min(lbA0, 0) + min(lbA1, 0) - 2 bound) / (-2 bound) in fp64 in that order,
 * an infeasible child counting as +inf, bound the pool's bound of slots[i]; 1.0 when bound >= 0; NaN for a row without a live pair.
 * Then, walking the rows in order: a row with gnn_improvement < branching_threshold gets kw_decisions[i] = the decision of
 * kw_score_conv.py:115-156 (fp32 values compared after promotion to double; the first maximum / minimum of a layer; between layers the
 * maximum of the tuples (value, index)), the counter *icp carried from row to row; every other row, a row whose scores or intercepts hold
 * a NaN and a row without an undecided node get [-1, -1] and leave the counter alone.  A row with a KW decision whose node's count in
 * ineff is below kwbd_threshold is SELECTED: sel_rows / sel_slots (K) and sel_decisions (K, 2) receive its row, slot and KW decision,
 * densely and in row order, *m their number.  All outputs are device arrays; workspace: gnnb_frontier_fallback_workspace_bytes. */
size_t gnnb_frontier_fallback_workspace_bytes(const gnnb_t* h, int K);
int gnnb_frontier_fallback(gnnb_t* h, const gnnb_pool* pool, const int32_t* slots, int K, const gnnb_fallback* in, double* gnn_improvement,
                           int32_t* kw_decisions, int32_t* sel_rows, int32_t* sel_slots, int32_t* sel_decisions, int32_t* m,
                           void* workspace, size_t workspace_bytes, void* stream);

/* gnnb_children whose rows gnnb_frontier_choose overwrites. */
typedef struct {
  int8_t* mask;
  double* const* lb;
  double* const* ub;
  int32_t* infeasible;
  double* bound;
  double* alpha;
  double* beta;
  double* ub_value;
  int32_t* live;
  int32_t n_graph;
} gnnb_children_rw;

/* m (0..K, the host's copy of *m): the selected parents; pair_b: their 2m children, rows 2j and 2j+1 those of sel_rows[j], bounded like
 * pair A after gnnb_frontier_expand on (sel_slots, sel_decisions).  Per selected parent kw_improvement = the formula above on pair B, then
 * bab_caller.resolve_branching: kw < gnn and kw < 0.05 adds 1 to ineff[node] (by one thread, in row order: two parents naming one node both
 * count); kw > gnn copies rows 2j, 2j+1 of pair_b over rows 2 sel_rows[j], + 1 of pair_a (mask, lb / ub of every graph layer, infeasible,
 * bound, alpha, beta, ub_value, live) and makes the KW decision the row's; otherwise pair A stays.  Writes for every row of K:
 * kw_improvement (-1.0 unless selected), used_kw (0 / 1) and decisions (K, 2) (gnn_decisions unless the KW pair was taken).  With m = 0
 * pair_b is not read.  sel_rows must be distinct rows of [0, K). */
int gnnb_frontier_choose(gnnb_t* h, const gnnb_pool* pool, int K, int m, const int32_t* sel_rows, const int32_t* sel_slots,
                         const int32_t* sel_decisions, const int32_t* gnn_decisions, const double* gnn_improvement,
                         const gnnb_children_rw* pair_a, const gnnb_children* pair_b, int32_t* ineff, double* kw_improvement,
                         int32_t* used_kw, int32_t* decisions, void* stream);

/* ---- the fall-back for many jobs in one pool (gnn_branching_amd/frontier.py verify_properties_threshold) ----
 * The two steps above per plan entry {segment, row0, k} of a gnnb_plan: every job has its own intercept counter and its own table of
 * inefficient points, so in the gnnb_fallback of these entry points icp is device (segments) and ineff device (segments, R) (both the
 * caller zeroes when a job takes a segment); the thresholds, sparsest_layer and random_order are the run's, the same for every job.  Per
 * entry the result is exactly gnnb_frontier_fallback's / gnnb_frontier_choose's on the rows [row0, row0 + k) with icp[segment] and
 * ineff[segment]: nothing mixes two entries, and a segment without an entry is not touched.  Refused with GNNB_E_INVALID before any launch:
 * everything the plan checks of section 7.4 refuse, gnnb_frontier_fallback's argument and range checks, M < 0 or M > n, a null array, a
 * network past the 4096-node cap; GNNB_E_STATE before gnnb_bind_network, GNNB_E_NOMEM for a short workspace.  Stream-ordered, no
 * allocation, no synchronisation, no atomics, no kernel waits on another workgroup; the prefix over the entries is a fixed order.
 *
 * gnnb_frontier_fallback_jobs: slots (n) global slot numbers; in: pair A's 2n rows, the parents' n rows of scores / intercepts /
 * scorer_mask.  gnn_improvement (n) and kw_decisions (n, 2) are indexed by global row.  The selected parents of all entries form ONE dense
 * list, in plan-entry order and within an entry in row order: sel_rows (n) holds GLOBAL rows, sel_slots (n) global slots, sel_decisions
 * (n, 2) the KW decisions; entry e occupies [sel0_e, sel0_e + m_e), sel0 the exclusive prefix sum of m over the entries in plan order.
 * m_entry: device (n_entries + 1) int32, m_e per entry, then M = their sum.  Entries of the lists from M on are not written.  The boxes
 * and property rows of pair B's child rows 2q and 2q + 1 (q < M) are copied from seg_x_lo / seg_x_hi (segments, N_0), seg_prop_w
 * (segments, N_L), seg_prop_b (segments) by the selected parent's segment into b_x_lo / b_x_hi (2n, N_0), b_prop_w (2n, N_L), b_prop_b
 * (2n): the host needs M (one read of m_entry) only for the launches behind -- gnnb_frontier_expand with K = M on (sel_slots,
 * sel_decisions), gnnb_kw_bounds / gnnb_dual_ascent / gnnb_net_eval with B = 2M -- and launches none of them, nor the choice, with M = 0. */
size_t gnnb_frontier_fallback_jobs_workspace_bytes(const gnnb_t* h, int n);
int gnnb_frontier_fallback_jobs(gnnb_t* h, const gnnb_pool* pool, const gnnb_plan* plan, const int32_t* slots, const gnnb_fallback* in,
                                const double* seg_x_lo, const double* seg_x_hi, const float* seg_prop_w, const float* seg_prop_b,
                                double* gnn_improvement, int32_t* kw_decisions, int32_t* sel_rows, int32_t* sel_slots, int32_t* sel_decisions,
                                int32_t* m_entry, double* b_x_lo, double* b_x_hi, float* b_prop_w, float* b_prop_b, void* workspace,
                                size_t workspace_bytes, void* stream);

/* gnnb_frontier_choose per entry on its m_e selected parents (its range of the dense lists, pair_b's rows 2q, 2q + 1) with ineff[segment]
 * (ineff: device (segments, R)), updated by one thread in row order; then pair B's rows are copied over pair A's for the parents that took
 * the KW pair.  M: the host's copy of m_entry[n_entries]; pair_a: the 2n rows; pair_b: 2M rows (not read with M = 0).  Writes
 * kw_improvement (n), used_kw (n) and decisions (n, 2) for every row of every entry. */
int gnnb_frontier_choose_jobs(gnnb_t* h, const gnnb_pool* pool, const gnnb_plan* plan, int M, const int32_t* m_entry, const int32_t* sel_rows,
                              const int32_t* sel_slots, const int32_t* sel_decisions, const int32_t* gnn_decisions,
                              const double* gnn_improvement, const gnnb_children_rw* pair_a, const gnnb_children* pair_b, int32_t* ineff,
                              double* kw_improvement, int32_t* used_kw, int32_t* decisions, void* stream);

/* ---- BaBSR alone: the decision of every parent row (gnn_branching_amd/frontier.py branching="babsr") ----
 * The branching of reference plnn/relu_conv_any_kw.py:45-181 with split_decision = 'kw' (relu_bab): every parent of a round gets the
 * decision of plnn/kw_score_conv.py:115-156 and one intercept counter is carried through the run (:100, :113).  scores / intercepts /
 * scorer_mask: device (K, R) fp32 as gnnb_babsr and gnnb_frontier_gather write them.  The rows are walked in order by one thread with the
 * counter *icp carried from row to row, and row i gets exactly what gnnb_frontier_fallback gives a row below its branching threshold:
 * the score decision if its layer is not sparsest_layer and its value, promoted to double, exceeds decision_threshold; otherwise the
 * intercept decision if some layer's minimum is below -1e-4 and the counter is below 2 (the LAST such layer; the counter becomes 0 unless
 * that layer is 0, then it is incremented); otherwise the first undecided node of the first layer, popping random_order (HOST, n_order
 * entries in 0..8) from its end, that has one (the counter becomes 0).  A row with a NaN in its scores or intercepts, a row without an
 * undecided node and a row for which random_order names no usable layer get [-1, -1] and leave the counter alone (gnnb_frontier_expand
 * makes two dead children of them and the commit closes the parent at its own bound; the host rule would raise).  There is no pair A, no
 * improvement, no table of inefficient points and no selection list.  The rule's text is the fall-back's: the same kernel reduces every
 * layer (k_frontier_candidates) and the same walk takes the three-way decision.  decisions: device (K, 2) int32; icp: device (1) int32,
 * read and updated; workspace: gnnb_frontier_babsr_decide_workspace_bytes (0 for a null or unbound handle).
 * Stream-ordered, no allocation, no synchronisation, no atomics, no workgroup waits on another; every arg-max / arg-min is the fixed tree
 * on the total order (value, index).  GNNB_E_INVALID before any launch for a null handle or argument, K outside 1..32767, n_order outside
 * 0..8, a NaN decision_threshold; GNNB_E_STATE before gnnb_bind_network; GNNB_E_NOMEM for a short workspace. */
size_t gnnb_frontier_babsr_decide_workspace_bytes(const gnnb_t* h, int K);
int gnnb_frontier_babsr_decide(gnnb_t* h, int K, const float* scores, const float* intercepts, const float* scorer_mask,
                               double decision_threshold, int sparsest_layer, const int32_t* random_order, int n_order, int32_t* icp,
                               int32_t* decisions, void* workspace, size_t workspace_bytes, void* stream);

/* gnnb_frontier_babsr_decide per plan entry {segment, row0, k} on the rows [row0, row0 + k) of the n-row arrays with the counter
 * icp[segment] (icp: device (segments); the caller zeroes it when a job takes the segment).  Nothing mixes two entries, a segment without
 * an entry is not touched, rows from n on are not written.  Also refused: everything the plan checks of section 7.4 refuse.  workspace:
 * gnnb_frontier_babsr_decide_workspace_bytes(h, n). */
int gnnb_frontier_babsr_decide_jobs(gnnb_t* h, const gnnb_plan* plan, const float* scores, const float* intercepts, const float* scorer_mask,
                                    double decision_threshold, int sparsest_layer, const int32_t* random_order, int n_order, int32_t* icp,
                                    int32_t* decisions, void* workspace, size_t workspace_bytes, void* stream);

/* ---- strong branching: bound every candidate split (gnn_branching_amd/frontier.py branching="strong") ----
 * The teacher of the GNN: for a parent row i of a round (pool slot slots[i], pool bound b, scorer_mask as gnnb_frontier_gather wrote it)
 * both children of every candidate ReLU are bounded and the row splits where the bound improves most.
 *
 * CANDIDATES (gnnb_strong_list).  top_m = 0: every node r with scorer_mask[i, r] != 0, in ascending flat ReLU index.  top_m = M > 0: the M
 * nodes of that set that come first in the total order (score descending, flat index ascending), emitted in ascending flat index; scores:
 * gnnb_babsr's, device (K, R) fp32, compared as float VALUES (-0.0 == +0.0: the index decides; +-inf are ordinary values); fewer than M
 * undecided nodes: all of them.  With top_m > 0 a row in which an undecided node's score is NaN gets no candidates (a NaN at a decided node
 * is ignored); a row whose slot is outside the pool gets none.  cand0: device (K + 1) int32, the exclusive prefix of the rows' counts in
 * row order, cand0[K] = n; the dense lists cand_row (n), cand_slot (n) and cand_dec (n, 2) as [layer, idx] -- cand_slot and cand_dec are
 * gnnb_frontier_expand's slots and decisions as they are.  Entries from n on are not written; the caller sizes the lists for
 * K * min(R, top_m or R) entries.  Two launches: k_strong_count (per row the count and, by bisection over the order-preserving integer key
 * of the float, the cut), k_strong_compact (the prefix over the K counts in row order, the row's candidates by a block scan in index order).
 * workspace: gnnb_strong_list_workspace_bytes (0 for a null or unbound handle).
 *
 * SCORE AND DECISION (gnnb_strong_pick).  live / infeasible / bound: device (2n), the candidates' children in list order (rows 2q blocked,
 * 2q + 1 passing) as gnnb_frontier_expand, gnnb_kw_bounds and gnnb_dual_ascent left them, in chunks of any size.  imp_q = b < 0 ?
 * (min(lb0, 0) + min(lb1, 0) - 2b) / (-2b) : 1.0, an infeasible child counting as +inf -- gnnb_frontier_fallback's formula, its operation
 * order; a candidate with a child row whose live == 0 has imp = NaN.  The decision of a row is the arg-max of imp over its candidates on
 * the total order (value descending, list position ascending), a fixed tree, NaN below every number; a row with no candidates or whose
 * every imp is NaN gets [-1, -1] (gnnb_frontier_expand makes two dead children of it and the commit closes the parent at its own bound).
 * Writes decisions (K, 2) int32 as gnnb_forward lays them out, best_improvement (K) fp64 (NaN without a decision), improvement (n) fp64
 * and, with table (NULL, or device (K, R) fp64), imp at (row, flat index) of every candidate and NaN everywhere else of the K rows.  n is
 * read from cand0[K] on the device.
 *
 * Both: stream-ordered, no allocation, no synchronisation, no atomics, no workgroup waits on another.  GNNB_E_INVALID before any launch for
 * a null handle or required argument, K outside 1..32767, top_m < 0, top_m > 0 with null scores, or a network past the 4096-node cap;
 * GNNB_E_STATE before gnnb_bind_network; GNNB_E_NOMEM for a short workspace. */
size_t gnnb_strong_list_workspace_bytes(const gnnb_t* h, int K);
int gnnb_strong_list(gnnb_t* h, const gnnb_pool* pool, const int32_t* slots, int K, const float* scorer_mask, const float* scores, int top_m,
                     int32_t* cand0, int32_t* cand_row, int32_t* cand_slot, int32_t* cand_dec, void* workspace, size_t workspace_bytes,
                     void* stream);
int gnnb_strong_pick(gnnb_t* h, const gnnb_pool* pool, const int32_t* slots, int K, const int32_t* cand0, const int32_t* cand_dec,
                     const int32_t* live, const int32_t* infeasible, const double* bound, int32_t* decisions, double* best_improvement,
                     double* improvement, double* table, void* stream);

/* The union of two shortlists (frontier.Shortlist(babsr=M, gnn=G)): the candidates of gnnb_strong_list from two
 * score arrays at once, e.g. gnnb_babsr's and gnnb_forward's scores_padded, so that a parent's table holds the scorer's own choice.
 *
 * THE RULE.  For row i let S_a be exactly the candidate set gnnb_strong_list gives for (scores_a, top_a): the first top_a undecided nodes
 * (scorer_mask[i, r] != 0) in the total order (score descending as float VALUES, flat index ascending; -0.0 == +0.0, +-inf are ordinary
 * values; fewer than top_a undecided nodes: all of them), and S_b the same for (scores_b, top_b).  The row's candidates are S_a u S_b,
 * each node once, emitted in ascending flat ReLU index.  cand_src[q] (device (n) int32, required) is 1 for a node in S_a only, 2 for one
 * in S_b only, 3 for one in both.  A NaN at an undecided node in EITHER array empties the row; a NaN at a decided node is ignored.  A row
 * whose slot is outside the pool gets no candidates, a row with no undecided node none.  cand0, cand_row, cand_slot and cand_dec mean what
 * they mean for gnnb_strong_list: cand0[K] = n, entries from n on are not written; the caller sizes the lists for
 * K * min(R, top_a + top_b) entries.
 *
 * Four launches: k_strong_count once per array (its bisection, one (mode, count, key, ties) record per row and array), then
 * k_strong_union_count (the walk over the row in tiles of 256 nodes with one running tie rank per array; the row's union count) and
 * k_strong_union_compact (k_strong_compact's prefix over the rows' counts in row order, the walk again, the entries).  The first three run
 * under the profile class k_strong_count, the last under k_strong_compact.  Stream-ordered, no allocation, no synchronisation, no atomics,
 * no workgroup waits on another; nothing depends on K or on a row's place.  GNNB_E_INVALID before any launch for a null handle or
 * required argument, K outside 1..32767, top_a < 1 or top_b < 1 (one list alone is gnnb_strong_list), or a network past the 4096-node cap;
 * GNNB_E_STATE before gnnb_bind_network; GNNB_E_NOMEM for a short workspace (gnnb_strong_list_union_workspace_bytes; 0 for a null or
 * unbound handle). */
size_t gnnb_strong_list_union_workspace_bytes(const gnnb_t* h, int K);
int gnnb_strong_list_union(gnnb_t* h, const gnnb_pool* pool, const int32_t* slots, int K, const float* scorer_mask, const float* scores_a,
                           int top_a, const float* scores_b, int top_b, int32_t* cand0, int32_t* cand_row, int32_t* cand_slot,
                           int32_t* cand_dec, int32_t* cand_src, void* workspace, size_t workspace_bytes, void* stream);

/* Strong branching for many jobs in one pool (frontier.verify_properties_strong): the boxes and property rows of a
 * chunk of c candidates, by the segment of their slot.  cand_slot: device (c) int32, a chunk of gnnb_strong_list's cand_slot; the pool is
 * `segments` segments of seg_cap slots and seg_x_lo / seg_x_hi (segments, N_0) fp64, seg_prop_w (segments, N_L) fp32, seg_prop_b
 * (segments) fp32 hold each segment's box and property row (as gnnb_frontier_fallback_jobs takes them).  Child rows 2q and 2q + 1 of
 * x_lo / x_hi (2c, N_0), prop_w (2c, N_L), prop_b (2c) receive the row of segment cand_slot[q] / seg_cap: plain copies, the ones
 * gnnb_frontier_fallback_jobs makes for pair B (one launch, under that copy's profile class k_frontier_rows_sel).  A slot < 0, or one whose
 * segment is >= segments, leaves its two rows unwritten and reads nothing out of bounds; gnnb_strong_list never lists such a slot.  Rows
 * from 2c on are not written.  Stream-ordered, no allocation, no synchronisation, no atomics, no workgroup waits on another.
 * GNNB_E_INVALID before any launch for c outside 1..32767, segments < 1 or seg_cap < 1 (before the handle is looked at), a null handle or
 * a null argument; GNNB_E_STATE before gnnb_bind_network. */
int gnnb_strong_rows_jobs(gnnb_t* h, const int32_t* cand_slot, int c, int segments, int seg_cap, const double* seg_x_lo,
                          const double* seg_x_hi, const float* seg_prop_w, const float* seg_prop_b, double* x_lo, double* x_hi, float* prop_w,
                          float* prop_b, void* stream);

/* ---- learning online inside the frontier (reference plnn/relu_conv_online.py:183-207) ----
 * The selection of the rows an online round learns from, after gnnb_frontier_choose: wrong (device (R) int32, zero at the start of a run)
 * is the reference's wrong_pts_dc, keyed by the flat ReLU index (the layer's offset + idx, graph_score_online.py:63-68) of the GNN's
 * decision.  One thread walks the K rows in order: a row with used_kw = 1 adds 1 to wrong[flat(gnn_decisions[i])]; when the count after
 * the increment is >= online_threshold the row is a LEARN row and learn_rows (its row), learn_kw (flat(kw_decisions[i])) and learn_imp
 * (1.0f if kw_improvement[i] - gnn_improvement[i] > 0.1, the difference in fp64, strictly greater, else 0.0f) receive it, densely and in row
 * order; *n_learn is their number.  Two rows that name one GNN node both count.  A row whose decisions name no node ([-1, -1]) or a node
 * outside its layer is never a learn row and leaves wrong alone.  Entries of the lists from *n_learn on are not written.  gnn_decisions /
 * kw_decisions: device (K, 2) int32 as gnnb_forward / gnnb_frontier_fallback wrote them; used_kw (K), gnn_improvement / kw_improvement (K)
 * as gnnb_frontier_choose and gnnb_frontier_fallback wrote them; learn_rows / learn_kw (K) int32, learn_imp (K) fp32, n_learn (1) int32.
 * Stream-ordered, no allocation, no synchronisation, no atomics.  GNNB_E_INVALID for a null handle or argument, K < 1, K > 32767 or
 * online_threshold < 1, GNNB_E_STATE before gnnb_bind_network -- all before the launch. */
int gnnb_frontier_learn(gnnb_t* h, int K, const int32_t* gnn_decisions, const int32_t* kw_decisions, const int32_t* used_kw,
                        const double* gnn_improvement, const double* kw_improvement, int online_threshold, int32_t* wrong,
                        int32_t* learn_rows, int32_t* learn_kw, float* learn_imp, int32_t* n_learn, void* stream);

/* ---- online learning for every job of a many-jobs round ----
 * gnnb_frontier_learn per plan entry {segment, row0, k}, after gnnb_frontier_choose_jobs: on the entry's rows [row0, row0 + k), in row order,
 * exactly the walk above against the segment's own table wrong[segment] (wrong: device (segments, R) int32; a segment's row is zero when
 * its job is admitted).  The learn rows of all entries form ONE dense list, in plan-entry order and within an entry in row order:
 * learn_rows holds GLOBAL row numbers (row0 + i, rows of the n-row parent batch), learn_kw and learn_imp as above (device (n) each), and
 * learn_entry (device (n_entries + 1) int32) the count of every entry followed by their sum N.  Entries of the lists from N on are not
 * written.  An entry's slice and its table do not depend on the other entries, their number or their order.  workspace: at least
 * gnnb_frontier_learn_jobs_workspace_bytes(h, n) bytes (0 for a null or unbound handle or n < 1), the entries' staging lists.
 * Stream-ordered, no allocation, no synchronisation, no atomics, no workgroup waits on another.  Before any launch: GNNB_E_INVALID for
 * everything the plan checks refuse (a null plan, no entry, n outside 1..32767, a null handle, entries that do not tile the rows),
 * online_threshold < 1 or a null argument, GNNB_E_NOMEM for a short workspace, GNNB_E_STATE before gnnb_bind_network. */
size_t gnnb_frontier_learn_jobs_workspace_bytes(const gnnb_t* h, int n);
int gnnb_frontier_learn_jobs(gnnb_t* h, const gnnb_plan* plan, const int32_t* gnn_decisions, const int32_t* kw_decisions,
                             const int32_t* used_kw, const double* gnn_improvement, const double* kw_improvement, int online_threshold,
                             int32_t* wrong, int32_t* learn_rows, int32_t* learn_kw, float* learn_imp, int32_t* learn_entry, void* workspace,
                             size_t workspace_bytes, void* stream);

/* ---- the witness of the upper bound ----
 * Every loop of the reference returns global_ub_point next to global_ub (plnn/branch_and_bound.py:157, plnn/relu_conv_gnnkwthreshold.py:
 * 209-214 and :268, plnn/relu_conv_online.py:225-228 and :276; experiments/bab_mip.py:50 stores it).  gnnb_frontier_witness keeps that point
 * on the device: it runs after the choice and before gnnb_frontier_commit, on the child rows the commit will see, takes the minimum of
 * ub_value over the live, feasible children on the total order (value, child index) -- a fixed tree with fmin semantics, a NaN never
 * wins -- and, if that minimum is strictly below *best_value, copies the child's N_0 floats to best_point and writes *best_value.  The
 * child's point is row c of x_a, unless used_kw[c >> 1] is set: then it is row 2j + (c & 1) of x_b with sel_rows[j] == c >> 1.  The caller
 * starts best_value at +inf; after every commit *best_value is the state record's global upper bound, bit for bit.
 * best_value: device (1) fp64 ((segments) in the jobs form); best_point: device (N_0) fp32 ((segments, N_0)).  children: the 2K rows
 * (only live, infeasible and ub_value are read).  Stream-ordered, no allocation, no synchronisation, no atomics.  GNNB_E_INVALID before
 * the launch for a null handle or argument, K outside 1..32767, m < 0 or m > K, used_kw with m > 0 but no x_b / sel_rows; GNNB_E_STATE
 * before gnnb_bind_network. */
typedef struct {
  const float* x_a;            /* (2K, N_0): the points ub_value of pair A's rows was evaluated at      */
  const float* x_b;            /* NULL, or pair B's (2m, N_0)                                          */
  const int32_t* used_kw;      /* NULL, or (K) as gnnb_frontier_choose wrote it                        */
  const int32_t* sel_rows;     /* NULL, or (m): row j of pair B belongs to parent row sel_rows[j]      */
  int32_t m;
} gnnb_witness_src;
int gnnb_frontier_witness(gnnb_t* h, int K, const gnnb_children* children, const gnnb_witness_src* src, double* best_value,
                          float* best_point, void* stream);

/* gnnb_frontier_witness per plan entry {segment, row0, k} on its children (rows [2 row0, 2 row0 + 2k) of the 2n), with its range
 * [sel0_e, sel0_e + m_e) of the dense lists (m_entry: device (n_entries + 1) as gnnb_frontier_fallback_jobs wrote it; M: the host's copy
 * of their sum; src->m is not read; m_entry may be NULL when M = 0 or used_kw is NULL), on best_value[segment] and best_point[segment].
 * Segments without an entry are not touched and nothing mixes two entries.  Refused like gnnb_frontier_witness, and for everything the
 * plan checks of section 7.4 refuse and for M < 0 or M > n. */
int gnnb_frontier_witness_jobs(gnnb_t* h, const gnnb_plan* plan, int M, const int32_t* m_entry, const gnnb_children* children,
                               const gnnb_witness_src* src, double* best_value, float* best_point, void* stream);

int gnnb_destroy(gnnb_t* h);

/* ---- online learning (reference graphnet/graph_score_online.py) ----
 * gnnb_get_weights / gnnb_set_weights: the 117 825 GNN parameters in gnnb_create's blob order (HOST) -- the
 * state_dict()/load_state_dict() of the model GraphChoice holds (graph_score_online.py:11-14).  set_weights rebuilds the
 * scorer's operand packs (device-synchronising). */
int gnnb_get_weights(const gnnb_t* h, float* w_blob, size_t n_floats);
int gnnb_set_weights(gnnb_t* h, const float* w_blob, size_t n_floats);

/* torch.optim.Adam(model.parameters(), lr=lr, weight_decay=wd) of graph_score_online.py:15 (betas 0.9/0.999, eps 1e-8,
 * moments start at zero).  Calling it again resets the optimizer state. */
int gnnb_online_create(gnnb_t* h, float lr, float weight_decay);

/* ---- where the scorer's operand packs are rebuilt after a learning step ----
 * gnnb_online_set_repack: mode 0 (the default; gnnb_online_create resets to it) is the host builder: a step with apply = 1 copies the
 * parameters to the host, synchronises, folds and permutes them into the 14 packs there and copies the packs back.  Mode 1 is the device
 * builder: two launches on the step's stream (k_repack_fold, k_repack_emit) read the trainer's parameters and rewrite the packs in
 * place; no parameter and no pack crosses the link.  The two builders run the same sums (fp64 accumulator, k ascending, rounded to
 * fp32 at the same points); every copied or permuted value is bit-identical, a folded entry may differ by one fp32 unit in the last
 * place.  Switching to mode 1 rebuilds the packs from the trainer's parameters at once (back to 0: with the host builder), so a handle's
 * packs always come from its mode's builder; both switches synchronise the device.  GNNB_E_INVALID for a null handle or a mode other than
 * 0 and 1, GNNB_E_STATE before gnnb_online_create.
 * In mode 1:
 *   - gnnb_online_step_rows and gnnb_imitation_step_rows with apply = 1 end with the Adam step followed by the pack rebuild on `stream`
 *     and return WITHOUT synchronising: loss, report_i, regret and status are device arrays, valid once `stream` reaches that point.  A
 *     second step may be issued on the same stream at once; the step keeps nothing on the host that the next would overwrite.
 *   - gnnb_online_step still synchronises `stream` (its loss is a host array) but moves no parameters or packs over the link.
 *   - gnnb_set_weights copies the blob to the trainer and runs the device builder; gnnb_get_weights synchronises the device and reads the
 *     parameters back from the trainer (the handle's host copy is stale after a step).
 * Ordering rule: the packs are rewritten IN PLACE on `stream`.  A gnnb_forward (or any other scorer call) of the same handle on another
 * stream must be ordered behind the step by the caller (an event, or a synchronise); on the same stream the order is the stream's.
 * gnnb_repack: the device builder alone, from the trainer's parameters, on `stream`; stream-ordered, allocates nothing, does not
 * synchronise.  GNNB_E_STATE before gnnb_online_create.
 * gnnb_pack_image: inspection.  Pack `which` (0..13: embed, pre_fwd, pre_bwd, pre_inp, prop, upd_fwd_e, upd_fwd_i, upd_fwd_f, upd_bwd,
 * upd_bwd_b, upd_inp, post_inp, score_b, score_f) as it stands in device memory, after a device synchronise, into host_buf (cap floats);
 * *n_floats (may be NULL) receives the pack's size whenever `which` is valid; a null host_buf with cap = 0 and a non-null n_floats is a
 * size query and succeeds without touching the device.  GNNB_E_INVALID for a null handle, any other null buffer, `which` outside 0..13,
 * or cap below the size. */
int gnnb_online_set_repack(gnnb_t* h, int mode);
int gnnb_repack(gnnb_t* h, void* stream);
int gnnb_pack_image(const gnnb_t* h, int which, float* host_buf, size_t cap, size_t* n_floats);
/* Inspection: fills the handle's pack block with NaNs (every byte 0xff), device-synchronising -- so that a test of a pack builder shows
 * that it writes every float.  The scorer is unusable until the packs are rebuilt (gnnb_set_weights, gnnb_repack). */
int gnnb_debug_poison_packs(gnnb_t* h);

/* GraphChoice.online_learning (graph_score_online.py:62-77) for B subproblems (the reference: B = 1; B > 1 sums the B
 * losses):  loss_b = max_j scores_b[j] - scores_b[kw_b] + improvement_b;  backward through GraphNet.forward;  one Adam step;
 * the scorer (gnnb_forward) uses the new parameters from the next call on.
 * in: the batch as for gnnb_forward (device pointers).  kw_index: HOST (B), the KW decision as a flat index into the R ReLU
 * nodes (trans_len[lay-1] + idx, :63-67) -- must be an undecided node of the mask.  A sample whose mask is empty (no score
 * to take the maximum of) gets loss = NaN and contributes nothing to the gradient; the other samples of the batch are not
 * affected.  improvement: HOST (B).  loss: HOST (B)
 * or NULL.  scores_padded: DEVICE (B, R) or NULL, the scores of the training-form forward before the update.  apply = 0:
 * compute the gradient only (read it with gnnb_online_grad), parameters and optimizer state untouched.
 * Limit: a convolution of the bound network may give one node at most 512 taps in either direction
 * (min(kh, H_in) min(kw, W_in) C_in forward, ceil(kh / stride) ceil(kw / stride) C_out transposed; 4x4 stride 2 over 32
 * channels: 512 / 128).  A network beyond it is refused with GNNB_E_INVALID before anything is launched; the handle stays usable.
 * Synchronises `stream` before returning. */
int gnnb_online_step(gnnb_t* h, const gnnb_batch* in, int B, const int32_t* kw_index, const float* improvement,
                     float* loss, float* scores_padded, int apply, void* stream);

/* gnnb_online_step on the rows rows[0..n) of the K-row DEVICE batch `in`, in list order, with nothing crossing the link: rows (device (n)
 * int32), kw_index (device (n) int32), improvement (device (n) fp32), loss (device (n) fp32 or NULL), status (device int32[1] the caller
 * zeroed, or NULL).  The listed rows of every tensor the step reads (the bounds of every graph layer, dual, the primals it reads, x_lp,
 * prop_w, prop_b, mask) are first copied into dense n-row buffers that belong to the handle; then the step runs at B = n: loss, gradient
 * and parameters are the bits of gnnb_online_step on the same rows given as a compact batch.  `in` is not written.
 * A device-fed index is checked on the device: a kw_index outside [0, R) or naming a node whose mask entry is 0, and a rows entry outside
 * [0, K), give that row loss = NaN and no gradient and set status bit 3 (value 8); nothing is read out of bounds and the other rows are not
 * affected (a rows entry that names no row is skipped: its sample runs on row 0's inputs under an empty mask).  GNNB_E_INVALID for n < 1 or n > K, a null handle or argument and gnnb_online_step's limits (taps, 8 ReLU layers, a
 * zero-tap network); GNNB_E_STATE before gnnb_bind_network or gnnb_online_create.  In repack mode 0 (the default) it synchronises `stream`
 * before returning, where gnnb_online_step does (the scorer's packs are rebuilt on the host from the new parameters); in mode 1 with
 * apply = 1 it does not synchronise (gnnb_online_set_repack above).  Inside a frontier run a learning round is
 * rare by construction -- a GNN node has to lose online_threshold times first -- and every other round stays free of it. */
int gnnb_online_step_rows(gnnb_t* h, const gnnb_batch* in, int K, const int32_t* rows, int n, const int32_t* kw_index, const float* improvement,
                          float* loss, int32_t* status, int apply, void* stream);

/* ---- the imitation step: learn the scorer from a strong-branching table ----
 * gnnb_online_step_rows under another loss.  The reference tree holds no supervised training script, so the loss is this library's own:
 * the online loss generalised from one named node to a whole table row, a margin-rescaled ranking hinge.  Per listed row, with s the
 * training-form scores (fp32 over the R flat ReLU indices, -inf at decided nodes), tau the row of `table` (fp64, NaN = not a
 * candidate: exactly what gnnb_strong_pick writes into its `table`) and margin >= 0:
 *   C = { r : tau[r] is not NaN };  t = arg-max of tau over C on (value descending, flat index ascending): the teacher;
 *   for q in C, q != t:  delta_q = (float)(margin (tau[t] - tau[q])) (fp64 product, rounded once);  term_q = (s[q] - s[t]) + delta_q in fp32;
 *   q is a violator iff term_q > 0;  loss = (float) sum over the violators of (double) term_q, in a fixed order;
 *   d loss / d s[q] = +1 per violator, d loss / d s[t] = - the number of violators.
 * A candidate whose mask entry is 0 or whose tau is +-inf refuses the row: loss = NaN, no gradient, status bit 3 (value 8).  A row without
 * a candidate: loss = NaN, no gradient, NO status bit.  One candidate: loss = 0, no gradient.  n > 1 sums the row losses un-normalised
 * (every d loss / d s entry is a small integer, so the gradient of fscore.bias is exactly 0).  If no row has a violator the gradient is
 * zero and apply = 1 still takes the Adam step: weight decay alone moves the parameters.
 * rows (n) int32, table (K, R) fp64 with row = batch row, loss (n) fp32 or NULL, report_i (n, 4) int32 or NULL = [teacher, pick, n_cand,
 * n_viol] (pick: the arg-max of s over C, value descending, index ascending), regret (n) fp64 or NULL = tau[teacher] - tau[pick], status
 * int32[1] zeroed by the caller or NULL: all DEVICE memory.  A refused or empty row reports -1, -1, 0, 0 and regret NaN.  Everything else --
 * the gather, the guards on `rows`, apply, the limits, the error codes, where it synchronises -- is gnnb_online_step_rows; loss, gradient
 * (gnnb_online_grad) and parameters are the bits of the same call on those rows given as a compact batch.  GNNB_E_INVALID also for a
 * margin that is negative or NaN. */
int gnnb_imitation_step_rows(gnnb_t* h, const gnnb_batch* in, int K, const int32_t* rows, int n, const double* table, double margin,
                             float* loss, int32_t* report_i, double* regret, int32_t* status, int apply, void* stream);

/* Inspection: the loss rule above alone, on caller-owned DEVICE arrays: scores and mask (n, R) fp32, table (n, R) fp64, ds (n, R) fp32
 * zeroed by the caller (receives d loss / d s; entries that are neither a violator nor the teacher are not written); loss, report_i,
 * regret, status as above.  Needs a bound handle (for R) and no trainer; stream-ordered, does not synchronise. */
int gnnb_imitation_loss(gnnb_t* h, const float* scores, const float* mask, const double* table, int n, double margin, float* loss, float* ds,
                        int32_t* report_i, double* regret, int32_t* status, void* stream);

/* ---- the replay buffer: learn the scorer from stored strong tables ----
 * A labelled state -- a row of a scorer batch and its row of gnnb_strong_pick's table -- is worth more than the one step of the round that
 * made it.  A replay BUFFER is caller-owned DEVICE memory: a gnnb_batch of C rows (of every tensor gnnb_imitation_step_rows reads: the
 * bounds of every graph layer, dual, the primals on either side of a ReLU layer and the last, x_lp, prop_w, prop_b, mask; any other
 * primal entry needs a non-null pointer that is never read), a table (C, R) fp64 and a state word int32[4] = {head, filled, stored,
 * skipped} that the caller zeroes once.  The step on a minibatch is the existing gnnb_imitation_step_rows(h, &buffer, C, idx, n,
 * buffer_table, ...): its workspaces scale with n, never with C.
 *
 * gnnb_replay_push: of the rows rows[0..n) (device int32, in list order) of the K-row device batch `src` and its table src_table (K, R),
 * row i is STORED iff its table row has at least two candidates (entries that are not NaN), every candidate is finite and every candidate
 * names an undecided node of the row's mask.  A row with 0 or 1 candidates is skipped silently (a step gets no gradient from it).  A row
 * the step would refuse (a candidate at a decided node, tau = +-inf) and a rows entry outside [0, K) are skipped and set bit 3 (value 8)
 * of *status (device int32[1] or NULL).  The r-th stored row of the call goes to slot (head + r) mod C; then head = (head + stored) mod C,
 * filled = min(C, filled + stored), and stored / skipped hold the call's counts.  No other slot is written.  Two launches (k_replay_rank,
 * k_replay_store) on `stream`, no synchronisation, no trainer needed (a bound handle collects).  GNNB_E_INVALID, before any launch, for C
 * outside 1..65536, K < 1, n < 1, n > K, n > C, a null handle or argument, and whatever gnnb_online_step_rows' batch check refuses of `src`
 * or `dst`; GNNB_E_STATE before gnnb_bind_network.
 *
 * gnnb_replay_sample: idx (device int32 (n), 1 <= n <= 256) receives min(n, filled) DISTINCT slots of [0, filled), `filled` read from the
 * device state word, and -1 in the entries beyond (the step skips such a row, with status bit 3).  A pure function of (filled, n, seed,
 * draw): with ns_mix the splitmix64 finaliser and G = 0x9E3779B97F4A7C15,
 *   base = ns_mix(seed ^ ns_mix(draw + 1));  key_j = ns_mix(base + G (j + 1))  (mod 2^64);
 *   idx = the j in [0, filled) with the smallest (key_j, j), in ascending order of (key_j, j).
 * One launch of one workgroup on `stream`, no synchronisation.  GNNB_E_INVALID for C outside 1..65536, n outside 1..256, a null handle or
 * argument.
 *
 * gnnb_replay_bytes: the bytes of a buffer's batch tensors and table for C slots on the bound network (the state word not counted);
 * 0 for a null or unbound handle or a C outside 1..65536. */
size_t gnnb_replay_bytes(const gnnb_t* h, int C);
int gnnb_replay_push(gnnb_t* h, const gnnb_batch* src, int K, const double* src_table, const int32_t* rows, int n, const gnnb_batch* dst, int C,
                     double* dst_table, int32_t* state, int32_t* status, void* stream);
int gnnb_replay_sample(gnnb_t* h, const int32_t* state, int C, int n, uint64_t seed, uint64_t draw, int32_t* idx, void* stream);

/* d loss / d parameters of the last gnnb_online_step, gnnb_online_step_rows or gnnb_imitation_step_rows (before weight decay), HOST, blob order.
 * In repack mode 1, where a step may only have been issued, it synchronises the device first. */
int gnnb_online_grad(const gnnb_t* h, float* grad, size_t n_floats);

const char* gnnb_last_error(void);
int gnnb_abi_version(void);
/* 32 hex digits: hash of the sources (and compiler flags) the library was built from; the Python loader compares it with the
 * tree's and refuses a stale binary. */
const char* gnnb_build_id(void);

/* ---- inspection hooks used by the parity tests and bench.py (not needed by a caller) ---- */

/* JSON text describing the launch plan of one forward for the bound network: per half-pass update the
 * kernel used, the tile shape of the MFMA gather (channels x pixel block, window, k-steps) and node counts. */
int gnnb_describe(const gnnb_t* h, char* buf, size_t cap);

/* Location of embedding mu[k] inside the workspace: row-major (B, N_k, p) fp32. */
int gnnb_mu_location(const gnnb_t* h, int B, int k, size_t* offset_bytes, size_t* n_floats);

/* Inspection: some producers store their embedding rows before their last Linear layer (the projection is folded into
 * the consumer): the rows of mu[k] left by the last forward are E with mu = W.E + b for Linear
 * `*linear_id` (index into the checkpoint's 26 Linear layers, state-dict order), or final when *linear_id = -1. */
int gnnb_mu_projection(const gnnb_t* h, int k, int* linear_id);

/* Stop after `n` half-passes (1 = round-0 forward sweep, 2 = + round-0 backward sweep, ...;
 * <= 0 = run everything).  With a limit set the scores are computed from the embeddings so far. */
int gnnb_set_halfpass_limit(gnnb_t* h, int n);

/* Occupy n_workgroups CUs (one workgroup per CU when lds_bytes > 80 KiB) for `ms` (<= 500) milliseconds on `stream` with a kernel that only
 * watches the clock: the test stand-in for "something else holds CUs while a forward runs" (a collective, a second batch). */
int gnnb_debug_occupy(int n_workgroups, int threads, size_t lds_bytes, double ms, void* stream);

/* Per-kernel-class timing with HIP events recorded on the launch stream.  When enabled every
 * launch in gnnb_forward is bracketed by a pair of events; gnnb_profile_read synchronises the
 * stream, accumulates and returns per class: total ms and launch count since the last reset. */
int gnnb_profile_enable(gnnb_t* h, int on);
int gnnb_profile_classes(void);                          /* number of classes */
const char* gnnb_profile_class_name(int cls);            /* kernel (class) name */
int gnnb_profile_read(gnnb_t* h, double* total_ms, int64_t* launches, int n, int reset);
/* The launches resolved by gnnb_profile_read since the previous call of this function, in launch order: class index and duration
 * (ms) of each.  Returns their number (>= 0; at most cap entries are written), or -1 for a null handle; clears the list. */
int gnnb_profile_trace(gnnb_t* h, int* cls, double* ms, int cap);

#ifdef __cplusplus
}
#endif
#endif /* GNNB_H */
