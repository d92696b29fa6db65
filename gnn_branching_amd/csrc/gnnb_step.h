// The learning step (`struct Step`, stage by stage, on the tape of gnnb_train.h) and its entry points, gnnb_online_create .. gnnb_imitation_loss.
// gnnb_online_step runs the stages on the caller's batch; the row forms begin the step, gather the listed rows into its arena, point
// the step at the gathered batch and run the rest.
// Included by gnnb.hip (one translation unit): it uses gnnb_handle, fail, HIPCHK, Launcher, refuse_batch, load_weights and repack_device.
#pragma once

// torch.optim.Adam(model.parameters(), lr, weight_decay) of graph_score_online.py:15; the moments start at zero
extern "C" int gnnb_online_create(gnnb_t* h, float lr, float weight_decay) {
  if (!h) return fail(GNNB_E_INVALID, "gnnb_online_create: null handle");
  if (int rc = fresh_blob(h)) return rc;           // (a trainer in repack mode 1 is being replaced: its parameters are the handle's)
  if (h->repack_mode == 1) {                       // the mode goes back to 0: the packs come from the host builder again
    HIPCHK(hipDeviceSynchronize());
    const std::vector<float> w(h->blob);
    if (int rc = load_weights(h, w.data(), nullptr)) return rc;
    h->repack_mode = 0;
  }
  if (!h->repack_segs.get()) {
    const std::vector<RepackSeg> segs = repack_segments(&h->repack_nblocks);
    for (const RepackSeg& s : segs)
      if (s.dst < 0 || (size_t)s.dst + repack_seg_floats(s) > h->pack_block.size())
        return fail(GNNB_E_INVALID, "gnnb_online_create: a pack segment ends outside the pack block");
    HIPCHK(h->repack_segs.upload(segs.data(), segs.size()));
    h->repack_nseg = (int)segs.size();
    HIPCHK(h->repack_scr.alloc(RepackScr::FLOATS));
    HIPCHK(hipMemset(h->repack_scr.get(), 0, RepackScr::FLOATS * sizeof(float)));
  }
  h->trainer.reset(new gnnb_train::Trainer());
  gnnb_train::Trainer* t = h->trainer.get();
  t->lr = lr; t->wd = weight_decay;
  const size_t n = blob_floats();
  for (DevBuf<float>* p : {&t->d_w, &t->d_g, &t->d_m, &t->d_v}) {
    HIPCHK(p->alloc(n));
    HIPCHK(hipMemset(p->get(), 0, n * sizeof(float)));
  }
  HIPCHK(hipMemcpy(t->d_w.get(), h->blob.data(), n * sizeof(float), hipMemcpyHostToDevice));
  HIPCHK(t->desc.alloc(gnnb_train::Trainer::kDescCap));
  for (int f = 0; f < gnnb_train::TILE_FORMS; ++f)       // the forward chain kernels stage a 192-wide layer: more than the default 64 KiB
    for (const LdsAttr& a : {LdsAttr(gnnb_train::kChainFwd[f], 96 * 1024), LdsAttr(gnnb_train::kChainFwdMulti[f], 96 * 1024)})
      HIPCHK(hipFuncSetAttribute(a.fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)a.bytes));
  return GNNB_OK;
}

extern "C" int gnnb_online_grad(const gnnb_t* h, float* grad, size_t n_floats) {
  if (!h || !grad || !h->trainer) return fail(GNNB_E_STATE, "gnnb_online_grad: no trainer (gnnb_online_create)");
  if (n_floats != blob_floats()) return fail(GNNB_E_INVALID, "gnnb_online_grad: %zu floats, expected %zu", n_floats, blob_floats());
  if (h->repack_mode == 1) HIPCHK(hipDeviceSynchronize());      // a mode-1 step may still be running on a stream the copy does not wait for
  HIPCHK(hipMemcpy(grad, h->trainer->d_g.get(), n_floats * sizeof(float), hipMemcpyDeviceToHost));
  return GNNB_OK;
}

// What gnnb_online_step and gnnb_online_step_rows check of the handle and of a batch of B before anything is launched.
static int online_preflight(gnnb_t* h, const gnnb_batch* in, int B, const char* who) {
  using namespace gnnb_train;
  if (!h->bound) return fail(GNNB_E_STATE, "%s: call gnnb_bind_network first", who);
  if (!h->trainer) return fail(GNNB_E_STATE, "%s: call gnnb_online_create first", who);
  const int L = (int)h->N.size() - 2;
  if (int rc = refuse_zero_taps(h, who)) return rc;
  if (int rc = refuse_batch(h, in, B, kNeedsOnline, who)) return rc;
  // k_tconv lists the valid taps of a destination node in LDS arrays of TCONV_MAXTAPS entries.  Both directions of every conv edge
  // run in a step (A and A^T, forward or as each other's adjoint): a node of A reads at most min(kh, H_in) min(kw, W_in) C_in
  // taps, a node of A^T at most min(ceil(kh / s), H_out) min(ceil(kw / s), W_out) C_out (the taps with (y + pad - ky) % s == 0).
  for (int k = 1; k <= L; ++k) {
    const Edge& e = h->edges[k];
    if (e.kind != 0) continue;
    auto lim = [](int a, int b) { return a < b ? a : b; };
    const long fwd = (long)lim(e.kh, e.h_in) * lim(e.kw, e.w_in) * e.c_in;
    const long bwd = (long)lim((e.kh + e.stride - 1) / e.stride, e.h_out) * lim((e.kw + e.stride - 1) / e.stride, e.w_out) * e.c_out;
    if (fwd > TCONV_MAXTAPS || bwd > TCONV_MAXTAPS)
      return fail(GNNB_E_INVALID, "%s: the convolution into ReLU layer %d (%dx%d stride %d, %d -> %d channels) gives a node up to %ld taps, "
                  "the training kernels hold %d", who, k, e.kh, e.kw, e.stride, e.c_in, e.c_out, fwd > bwd ? fwd : bwd, TCONV_MAXTAPS);
  }
  if (L > T_MAXL) return fail(GNNB_E_INVALID, "%s: more than %d ReLU layers", who, T_MAXL);
  return GNNB_OK;
}

// The loss of a step is a parameter: the KW form (d_kw (DEVICE, B): the KW decision as a flat index into the R ReLU nodes,
// trans_len[lay-1] + idx, graph_score_online.py:63-67; d_imp (DEVICE, B); k_tloss, k_tscore_bwd_w over its two nodes per sample) or the
// table form of gnnb_imitation_step_rows (table != null: k_tloss_table over the (B, R) fp64 rows, k_tscore_bwd_w_dense over the dense ds;
// report_i (B, 4) and regret (B), DEVICE, may be NULL).  Everything else is shared.
struct StepLoss {
  const int32_t* d_kw = nullptr; const float* d_imp = nullptr;                                            // KW form
  const double* table = nullptr; double margin = 0.0; int32_t* report_i = nullptr; double* regret = nullptr;      // table form
};
struct StepOut {                       // where a step's results go; each may be NULL
  float* loss_host = nullptr;          // HOST (B): asking for it makes the step wait for the stream
  float* loss_dev = nullptr;           // DEVICE (B)
  float* scores_padded = nullptr;      // DEVICE (B, R): the scores of the training-form forward BEFORE the update
  int32_t* status = nullptr;           // DEVICE int32[1]: bit 3 (value 8) of k_tloss / k_tloss_table / k_trows_gather
};

// One GraphChoice.online_learning step (graph_score_online.py:62-77) for B subproblems (the reference: B = 1):
//   loss = sum_b ( max_j scores_b[j] - scores_b[kw_b] + improvement_b );  backward;  Adam step;  scorer packs rebuilt.
// Behind online_preflight.  in: the batch exactly as for gnnb_forward.  apply = 0: gradient only (gnnb_online_grad), the parameters and
// the Adam state stay as they are.  finished: the caller returns a finished step whatever the repack mode (gnnb_online_step).
struct Step {
  gnnb_t* h; const gnnb_batch* in; int B; StepLoss lf; StepOut out; int apply; hipStream_t st; const char* who; bool finished;

  using Trainer = gnnb_train::Trainer; using Spec = Trainer::Spec; using TT = gnnb_train::TT; using TSeg = gnnb_train::TSeg;
  Trainer& t = *h->trainer;
  const int K = (int)h->N.size() - 1, L = K - 1, R = h->R, T = h->T;
  struct LC { float *r0, *r1, *amb, *live, *nd2, *d1, *ff, *fb; Trainer::List ambl, livel; };
  LC lc[T_MAXL + 1];                                       // per-node constants of ReLU layer k, and its two node lists
  const float *inp3 = nullptr, *inp2 = nullptr, *featp = nullptr;
  TT relax_f[T_MAXL + 1], relax_b[T_MAXL + 1], mu[T_MAXL + 2];
  long rows_of(int k) const { return (long)B * h->N[k]; }

  static TSeg S(const TT& x, const float* s = nullptr) { return TSeg{x.v, s, x.g, 0}; }           // a segment of a Linear: rows x, scaled by s
  static TSeg SF(const TT& x, const float* s = nullptr) { return TSeg{x.v, s, x.g, 1}; }          // ... addressed by node
  static TSeg P(const float* s = nullptr) { return TSeg{nullptr, s, nullptr, 0}; }                // ... the previous op of the chain

  // ---- begin: an empty tape, the arena back to zero (the row forms take their gathered rows out of it next), the edge weights ----
  int begin() {
    t.st = st;
    t.ordered = h->repack_mode == 1 && apply && !out.loss_host;      // this step is issued, not waited for (apply_and_sync)
    t.n_cu = h->n_cu;
    t.tape.clear();
    t.ndesc = 0;
    if (t.arena.reset(st)) return fail(GNNB_E_HIP, "%s: arena reset failed", who);
    if (h->edge_w.empty()) {                                 // torch-layout copies of the verified network's weights: they belong to the bound network
      std::vector<DevBuf<float>> ew(h->edges.size());
      for (int k = 1; k <= L; ++k) HIPCHK(ew[k].upload(h->edges[k].w.data(), h->edges[k].w.size()));
      h->edge_w = std::move(ew);
    }
    return GNNB_OK;
  }

  // ---- per-node constants: the step's own buffers zeroed, then k_tprep, the node lists, the feature rows ----
  int node_constants() {
    using namespace gnnb_train;
    HIPCHK(t.d_sel.grow((size_t)B * 2));
    HIPCHK(t.d_scores.grow((size_t)B * R));
    HIPCHK(t.d_ds.grow((size_t)B * R));
    HIPCHK(t.d_loss.grow(B));
    HIPCHK(hipMemsetAsync(t.d_ds.get(), 0, (size_t)B * R * 4, st));
    HIPCHK(hipMemsetAsync(t.d_g.get(), 0, blob_floats() * 4, st));
    TPrepMulti pm{};
    TCompactMulti cm{};
    long nmax = 0;
    for (int k = 1; k <= L; ++k) {
      const long n = rows_of(k);
      nmax = n > nmax ? n : nmax;
      LC& c = lc[k];
      for (float** p : {&c.r0, &c.r1, &c.amb, &c.live, &c.nd2, &c.d1}) *p = t.arena.alloc(n);
      c.ff = t.arena.alloc(7 * n);
      c.fb = t.arena.alloc(7 * n);
      // node lists: the relaxation chains run over the ambiguous nodes, the update chains over the live ones
      int* buf = reinterpret_cast<int*>(t.arena.alloc(2 * n + 2));
      if (t.arena.err || !buf) return fail(GNNB_E_NOMEM, "%s: out of device memory", who);
      const ReluRows r = relu_rows(*h, *in, B, k);
      pm.a[k - 1] = TPrepArgs{r.lb, r.ub, r.dual, r.z_pre, r.z_post, h->dev[k].bias.get(), h->N[k], h->hw[k], n,
                              c.r0, c.r1, c.amb, c.live, c.nd2, c.d1, c.ff, c.fb};
      c.ambl = Trainer::List{buf, buf + 2 * n, n};
      c.livel = Trainer::List{buf + n, buf + 2 * n + 1, n};
      cm.a[2 * (k - 1)] = TCompact{c.amb, buf, buf + 2 * n, n};
      cm.a[2 * (k - 1) + 1] = TCompact{c.live, buf + n, buf + 2 * n + 1, n};
    }
    hipLaunchKernelGGL(k_tprep, dim3((unsigned)((nmax + 255) / 256), (unsigned)L), dim3(256), 0, st, pm);      // every layer, one launch
    hipLaunchKernelGGL(k_tcompact, dim3((unsigned)(2 * L)), dim3(256), 0, st, cm);                              // every list, one launch
    const long n0 = rows_of(0);
    TColsMulti m{};
    auto job = [&](int j, std::initializer_list<const float*> cs, long n) {
      TColsArgs& a = m.a[j];
      int w = 0;
      for (const float* c : cs) a.c[w++] = c;
      a.w = w; a.n = n; a.dst = t.arena.alloc((size_t)n * w);
      return (const float*)a.dst;
    };
    inp3 = job(0, {in->lb[0], in->x_lp, in->ub[0]}, n0);                                                    // graph_conv.py:90-93
    inp2 = job(1, {in->lb[0], in->ub[0]}, n0);                                                              // :380-381
    featp = job(2, {in->lb[K], in->ub[K], in->primal[in->n_primal - 1], in->prop_b}, B);                   // :202-205
    hipLaunchKernelGGL(k_tcols, dim3((unsigned)(((n0 > B ? n0 : B) + 255) / 256), 3), dim3(256), 0, st, m);
    return GNNB_OK;
  }

  // ---- relaxation terms (graph_conv.py:153-161, :273-293): functions of the node features only, so the same in every round
  // -- computed once (the reference recomputes them per round; their gradient contributions from all rounds add up in
  // relax.g before the chain is walked back once) and only for the ambiguous nodes (`* amb` zeroes every other row).
  // Every layer's chain in one launch (Trainer::chain_multi).
  void relaxation() {
    std::vector<Trainer::Job> jf, jb;
    for (int k = 1; k <= L; ++k) {
      const LC& c = lc[k];
      jf.push_back({{Spec{L_FC1, {}, c.ff, true, nullptr, false},
                     Spec{L_FC1_1, {P()}, nullptr, false, c.amb, true}}, rows_of(k), &c.ambl});                   // :160-161
      jb.push_back({{Spec{L_BC1, {}, c.fb, true, nullptr, false},
                     Spec{L_BC1_1, {P()}, nullptr, true, nullptr, false},
                     Spec{L_BC1_2, {P()}, nullptr, false, nullptr, false},                                        // :285
                     Spec{L_BC2, {P(), P(c.nd2), P(c.d1)}, nullptr, true, nullptr, false},                        // :287-291
                     Spec{L_BC2_1, {P()}, nullptr, false, c.amb, true}}, rows_of(k), &c.ambl});                   // :293
    }
    const auto of = t.chain_multi(jf);
    const auto ob = t.chain_multi(jb);
    for (int k = 1; k <= L; ++k) { relax_f[k] = of[k - 1][1]; relax_b[k] = ob[k - 1][4]; }
  }

  // nb = A_k src (dir 0) or A_k^T src (dir 1, / tap count if norm), on the tape.  k = K: the property layer, one (1, N_L) matrix per sample.
  TT edge(int k, int dir, int norm, const TT& src) {
    using namespace gnnb_train;
    const Edge& e = h->edges[k < K ? k : L];               // (not read at k = K)
    TT y = t.rows(rows_of(dir == 0 ? k : k - 1));
    if (k == K)
      t.dense(TDense{in->prop_w, (long)h->N[L], src.v, y.v, B, 1, h->N[L], dir, 0}, src, y);
    else if (e.kind == 0)
      t.conv(TConv{src.v, y.v, h->edge_w[k].get(), B, e.c_in, e.h_in, e.w_in, e.c_out, e.h_out, e.w_out, e.kh, e.kw, e.stride, e.pad, dir, norm, 0}, src, y);
    else
      t.dense(TDense{h->edge_w[k].get(), 0, src.v, y.v, B, e.n_out, e.n_in, dir, 0}, src, y);
    return y;
  }

  // ---- the T rounds of graph_conv.py:77-388, every Linear on the tape; each MLP chain is one launch (Trainer::chain) ----
  void rounds() {
    const long n0 = rows_of(0);
    for (int r = 0; r < T; ++r) {
      if (r == 0)
        mu[0] = t.chain({Spec{L_INP_F, {}, inp3, true, nullptr, false}, Spec{L_INP_F_1, {P()}, nullptr, false, nullptr, false}}, n0)[1];   // :94
      for (int k = 1; k <= L; ++k) {                                                       // :107-192
        const LC& c = lc[k];
        TT nb = edge(k, 0, 0, mu[k - 1]);
        // the update chain over the live nodes only (`* live` zeroes the rows of the others, :178)
        mu[k] = t.chain({Spec{L_FC3, {SF(nb, c.r0), SF(nb, c.r1)}, nullptr, true, nullptr, false},                  // :169-170
                         Spec{L_FC3_2, {P()}, nullptr, false, nullptr, false},
                         Spec{L_FC4, {SF(relax_f[k]), P()}, nullptr, true, nullptr, false},                         // :176-177
                         Spec{L_FC4_2, {P()}, nullptr, false, c.live, true}}, rows_of(k), &c.livel)[3];             // :178
      }
      {                                                                                    // :194-210
        TT nb = edge(K, 0, 0, mu[L]);
        mu[K] = t.chain({Spec{L_OUT1, {}, featp, true, nullptr, false},
                         Spec{L_OUT2, {P(), S(nb)}, nullptr, true, nullptr, false},
                         Spec{L_OUT3, {P()}, nullptr, false, nullptr, false}}, B)[2];
      }
      for (int k = L; k >= 1; --k) {                                                       // :222-350
        const LC& c = lc[k];
        TT nb = edge(k + 1, 1, k < L && h->edges[k + 1].kind == 0 ? 1 : 0, mu[k + 1]);                          // :299-326
        mu[k] = t.chain({Spec{L_BC3, {SF(nb, c.r0), SF(nb, c.r1)}, nullptr, true, nullptr, false},                  // :331-336
                         Spec{L_BC3_1, {P()}, nullptr, false, nullptr, false},
                         Spec{L_BC4, {SF(relax_b[k]), P()}, nullptr, true, nullptr, false},                         // :344-345
                         Spec{L_BC4_1, {P()}, nullptr, false, c.live, true}}, rows_of(k), &c.livel)[3];             // :347
      }
      if (r + 1 < T) {                                                                     // :360-385 (the last round's input rows feed nothing)
        TT nb = edge(1, 1, 0, mu[1]);
        mu[0] = t.chain({Spec{L_INP_B, {}, inp2, true, nullptr, false},
                         Spec{L_INP_B_1, {P()}, nullptr, false, nullptr, false},
                         Spec{L_INP_B2, {P(), S(nb)}, nullptr, true, nullptr, false},
                         Spec{L_INP_B2_2, {P()}, nullptr, false, nullptr, false}}, n0)[3];
      }
    }
  }

  // ---- scores (:442-450) and the loss ----
  int scores_and_loss() {
    using namespace gnnb_train;
    float *const d_w = t.d_w.get(), *const d_g = t.d_g.get(), *const d_scores = t.d_scores.get(), *const d_ds = t.d_ds.get();
    std::vector<Trainer::Job> jn;
    for (int k = 1; k <= L; ++k) jn.push_back({{Spec{L_FNODE, {S(mu[k])}, nullptr, true, nullptr, false}}, rows_of(k), nullptr});
    const auto hk = t.chain_multi(jn);
    TScoreMulti sm{};
    int off = 0;
    long nmax = 0;
    for (int k = 1; k <= L; ++k) {
      const long n = rows_of(k);
      nmax = n > nmax ? n : nmax;
      sm.a[k - 1] = TScore{hk[k - 1][0].v, hk[k - 1][0].g, d_w + weight_offset(L_FSCORE), d_w + bias_offset(L_FSCORE), in->mask, d_scores,
                           d_ds, h->N[k], R, off, n, d_g + weight_offset(L_FSCORE), d_g + bias_offset(L_FSCORE), t.d_sel.get(), B};
      off += h->N[k];
    }
    const dim3 grid((unsigned)((nmax + 3) / 4), (unsigned)L);
    hipLaunchKernelGGL(k_tscore_fwd, grid, dim3(256), 0, st, sm);
    TScoreDense sd{};                                      // table form: the chunk partials of the dense fscore gradient
    if (lf.table) {
      for (int k = 1; k <= L; ++k) sd.part_off[k] = sd.part_off[k - 1] + (int)((rows_of(k) + TSD_CHUNK - 1) / TSD_CHUNK);
      sd.part = reinterpret_cast<double*>(t.arena.alloc((size_t)sd.part_off[L] * 65 * 2));      // (fp64 partials; the arena hands out 256-byte aligned blocks)
    }
    const bool dense = lf.table != nullptr;
    const dim3 dgrid((unsigned)((nmax + TSD_CHUNK - 1) / TSD_CHUNK), (unsigned)L);
    t.tape.push_back([sm, sd, grid, dgrid, dense, L = L, st = st]() {
      hipLaunchKernelGGL(k_tscore_bwd, grid, dim3(256), 0, st, sm);
      if (dense) {
        hipLaunchKernelGGL(k_tscore_bwd_w_dense, dgrid, dim3(256), 0, st, sm, sd);
        hipLaunchKernelGGL(k_tscore_reduce_dense, dim3(1), dim3(128), 0, st, sm, sd, L);
      } else {
        hipLaunchKernelGGL(k_tscore_bwd_w, dim3(1), dim3(64), 0, st, sm, L);
      }
    });
    if (t.arena.err) return fail(GNNB_E_NOMEM, "%s: out of device memory", who);
    if (out.scores_padded) HIPCHK(hipMemcpyAsync(out.scores_padded, d_scores, (size_t)B * R * 4, hipMemcpyDeviceToDevice, st));
    if (lf.table) {
      TLossTable la{d_scores, in->mask, lf.table, d_ds, t.d_loss.get(), lf.report_i, lf.regret, out.status, R, lf.margin};
      hipLaunchKernelGGL(k_tloss_table, dim3(B), dim3(256), 0, st, la);
    } else {
      TLoss la{d_scores, d_ds, lf.d_kw, lf.d_imp, t.d_loss.get(), R, t.d_sel.get(), in->mask, out.status};
      hipLaunchKernelGGL(k_tloss, dim3(B), dim3(256), 0, st, la);
    }
    return GNNB_OK;
  }

  // ---- backward: the tape in reverse, then the weight gradients of every op it recorded ----
  int backward() {
    t.wops.clear();
    for (auto it = t.tape.rbegin(); it != t.tape.rend(); ++it) (*it)();
    t.tape.clear();
    if (t.weight_grads()) return fail(GNNB_E_HIP, "%s: the weight-gradient launches failed", who);
    if (t.arena.err) return fail(GNNB_E_NOMEM, "%s: out of device memory", who);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(GNNB_E_HIP, "%s: a launch failed: %s", who, hipGetErrorString(e));
    return GNNB_OK;
  }

  // ---- the losses out, the Adam step, the scorer's packs, and when the call waits for the stream ----
  // The rules, all of them here:
  //   * apply = 0 waits (the caller reads the gradient next);
  //   * repack mode 0 waits after Adam: the host builder reads the new parameters, and load_weights uploads its packs;
  //   * repack mode 1 issues the device builder behind Adam and does not wait (t.ordered, decided in begin: host tables went through
  //     k_tput) -- unless a host loss was asked for, or the caller returns finished steps only (gnnb_online_step).
  int apply_and_sync() {
    using namespace gnnb_train;
    if (out.loss_host) {
      t.h_loss.resize(B);
      HIPCHK(hipMemcpyAsync(t.h_loss.data(), t.d_loss.get(), (size_t)B * 4, hipMemcpyDeviceToHost, st));
    }
    if (out.loss_dev) HIPCHK(hipMemcpyAsync(out.loss_dev, t.d_loss.get(), (size_t)B * 4, hipMemcpyDeviceToDevice, st));
    if (apply) {
      t.step += 1;
      const double b1 = 0.9, b2 = 0.999;
      const double bc1 = 1.0 - std::pow(b1, t.step), bc2 = 1.0 - std::pow(b2, t.step);
      TAdam a{t.d_w.get(), t.d_g.get(), t.d_m.get(), t.d_v.get(), (int)blob_floats(), (float)(t.lr / bc1), t.wd, (float)(1.0 - b1), (float)b2, (float)(1.0 - b2), 1e-8f, (float)std::sqrt(bc2)};
      hipLaunchKernelGGL(k_tadam, dim3((unsigned)((blob_floats() + 255) / 256)), dim3(256), 0, st, a);
      if (h->repack_mode == 1) {              // the packs follow on the stream; nothing crosses the link
        if (int rc = repack_device(h, st)) return rc;
        h->blob_stale = true;
        if (!t.ordered || finished) HIPCHK(hipStreamSynchronize(st));
      } else {
        std::vector<float> nw(blob_floats());
        HIPCHK(hipMemcpyAsync(nw.data(), t.d_w.get(), nw.size() * 4, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        if (int rc = load_weights(h, nw.data(), st)) return rc;      // the scorer's folded packs follow the new parameters
      }
    } else {
      HIPCHK(hipStreamSynchronize(st));
    }
    if (out.loss_host) memcpy(out.loss_host, t.h_loss.data(), (size_t)B * 4);
    return GNNB_OK;
  }

  int stages() {                         // everything behind begin
    int rc = node_constants();
    if (!rc) { relaxation(); rounds(); rc = scores_and_loss(); }
    if (!rc) rc = backward();
    return rc ? rc : apply_and_sync();
  }
};

// in: the batch exactly as for gnnb_forward.  kw_index (HOST, B), which must name an undecided node of the mask; improvement (HOST, B);
// loss (HOST, B, may be NULL): the host checks and the two small copies in front of the step.  Always returns a finished step.
extern "C" int gnnb_online_step(gnnb_t* h, const gnnb_batch* in, int B, const int32_t* kw_index, const float* improvement,
                                float* loss, float* scores_padded, int apply, void* stream) {
  const char* who = "gnnb_online_step";
  if (!h || !in || !kw_index || !improvement) return fail(GNNB_E_INVALID, "%s: null argument", who);
  if (int rc = online_preflight(h, in, B, who)) return rc;
  for (int b = 0; b < B; ++b)
    if (kw_index[b] < 0 || kw_index[b] >= h->R) return fail(GNNB_E_INVALID, "%s: kw_index[%d] = %d outside [0, %d)", who, b, kw_index[b], h->R);
  gnnb_train::Trainer& t = *h->trainer;
  hipStream_t st = (hipStream_t)stream;
  HIPCHK(t.d_imp.grow(B));
  HIPCHK(t.d_kw.grow(B));
  HIPCHK(hipMemcpyAsync(t.d_kw.get(), kw_index, (size_t)B * 4, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(t.d_imp.get(), improvement, (size_t)B * 4, hipMemcpyHostToDevice, st));
  Step s{h, in, B, StepLoss{t.d_kw.get(), t.d_imp.get()}, StepOut{loss, nullptr, scores_padded, nullptr}, apply, st, who, true};
  if (int rc = s.begin()) return rc;
  return s.stages();
}

// ---- THE list of the tensors a learning step reads of a batch on the bound network ----
// In this order: lb[k], ub[k] of every graph layer; per ReLU layer dual[k - 1] and the two primals on either side of it; the last primal;
// x_lp, prop_w, prop_b; the mask.  w: floats per row.  step_rows gathers exactly these rows, gnnb_replay_push stores exactly
// these rows and gnnb_replay_bytes adds up exactly these widths, so the three cannot drift apart.
enum { ST_LB, ST_UB, ST_DUAL, ST_PRIMAL, ST_XLP, ST_PROPW, ST_PROPB, ST_MASK };
struct StepTensor { int group, k; long w; };
static std::vector<StepTensor> step_tensors(const gnnb_t* h, int n_primal) {
  const int NG = (int)h->N.size(), L = NG - 2;
  std::vector<StepTensor> out;
  for (int k = 0; k < NG; ++k) { out.push_back({ST_LB, k, h->N[k]}); out.push_back({ST_UB, k, h->N[k]}); }
  std::vector<char> done(n_primal, 0);
  for (int k = 1; k <= L; ++k) {
    out.push_back({ST_DUAL, k - 1, 3L * h->N[k]});
    for (int q : {h->relu_q[k] - 1, h->relu_q[k]})
      if (!done[q]) { out.push_back({ST_PRIMAL, q, h->N[k]}); done[q] = 1; }
  }
  if (!done[n_primal - 1]) out.push_back({ST_PRIMAL, n_primal - 1, 1});
  out.push_back({ST_XLP, 0, h->N[0]});
  out.push_back({ST_PROPW, 0, h->N[L]});
  out.push_back({ST_PROPB, 0, 1});
  out.push_back({ST_MASK, 0, h->R});
  return out;
}
static const float* step_tensor(const gnnb_batch& b, const StepTensor& e) {
  const float* const* const tab[] = {b.lb, b.ub, b.dual, b.primal};
  const float* const one[] = {b.x_lp, b.prop_w, b.prop_b, b.mask};
  return e.group <= ST_PRIMAL ? tab[e.group][e.k] : one[e.group - ST_XLP];
}
// A batch whose pointer tables are its own copies, so that entries can be pointed elsewhere (`b` is the batch to hand on).
struct BatchView {
  std::vector<const float*> tab[4];      // lb, ub, dual, primal, by group
  gnnb_batch b;
  explicit BatchView(const gnnb_batch& in)
      : tab{{in.lb, in.lb + in.n_graph}, {in.ub, in.ub + in.n_graph}, {in.dual, in.dual + in.n_relu}, {in.primal, in.primal + in.n_primal}}, b(in) {
    b.lb = tab[ST_LB].data(); b.ub = tab[ST_UB].data(); b.dual = tab[ST_DUAL].data(); b.primal = tab[ST_PRIMAL].data();
  }
  BatchView(const BatchView&) = delete;
  void set(const StepTensor& e, const float* p) {
    const float** const one[] = {&b.x_lp, &b.prop_w, &b.prop_b, &b.mask};
    if (e.group <= ST_PRIMAL) tab[e.group][e.k] = p; else *one[e.group - ST_XLP] = p;
  }
};

// The body gnnb_online_step_rows and gnnb_imitation_step_rows share behind their checks.  s: the step at B = n on the K-row SOURCE batch,
// s.lf.table (table form) the (K, R) table of that batch: its listed rows are gathered with the other tensors (a fp64 row is 2 R floats).
static int step_rows(Step& s, int K, const int32_t* rows) {
  using namespace gnnb_train;
  gnnb_t* const h = s.h;
  const gnnb_batch* const in = s.in;
  Trainer& t = s.t;
  const int n = s.B, R = s.R;
  if (int rc = s.begin()) return rc;
  TGather g{};
  g.K = K; g.rows = rows; g.status = s.out.status;
  BatchView dn(*in);                                                    // (entries the step does not read stay)
  for (const StepTensor& e : step_tensors(h, in->n_primal)) {           // the n listed rows of every (K, w) tensor the step reads
    float* d = t.arena.alloc((size_t)n * e.w);
    if (e.group == ST_MASK) g.mask_t = g.nt;
    g.t[g.nt++] = TGatherT{step_tensor(*in, e), d, (int)e.w};
    dn.set(e, d);
  }
  if (s.lf.table) {
    float* d = t.arena.alloc((size_t)n * 2 * R);
    g.t[g.nt++] = TGatherT{reinterpret_cast<const float*>(s.lf.table), d, 2 * R};
    s.lf.table = reinterpret_cast<const double*>(d);
  }
  if (t.arena.err) return fail(GNNB_E_NOMEM, "%s: out of device memory", s.who);
  Launcher run{s.h, s.st};
  run.run(PC_TROWS_GATHER, [&] { hipLaunchKernelGGL(k_trows_gather, dim3(n, TG_SPLIT), dim3(TG_THREADS), 0, s.st, g); });
  if (run.rc) return run.rc;
  s.in = &dn.b;
  return s.stages();
}

// gnnb_online_step on the rows rows[0..n) of the K-row device batch `in`, in list order, nothing crossing the link: k_trows_gather copies
// the listed rows of every tensor the step reads into dense n-row buffers out of the trainer's arena, then the step runs at B = n
// on them.  Repack mode 0: synchronises where gnnb_online_step does.  Mode 1 with apply = 1: the step and the pack rebuild are issued on the
// stream and the call returns without synchronising (include/gnnb.h, gnnb_online_set_repack).
extern "C" int gnnb_online_step_rows(gnnb_t* h, const gnnb_batch* in, int K, const int32_t* rows, int n, const int32_t* kw_index,
                                     const float* improvement, float* loss, int32_t* status, int apply, void* stream) {
  const char* who = "gnnb_online_step_rows";
  if (K < 1 || n < 1 || n > K) return fail(GNNB_E_INVALID, "%s: n = %d rows of a batch of K = %d (1 <= n <= K)", who, n, K);
  if (!h) return fail(GNNB_E_INVALID, "%s: null handle", who);
  if (!in || !rows || !kw_index || !improvement) return fail(GNNB_E_INVALID, "%s: null argument", who);
  if (int rc = online_preflight(h, in, K, who)) return rc;
  Step s{h, in, n, StepLoss{kw_index, improvement}, StepOut{nullptr, loss, nullptr, status}, apply, (hipStream_t)stream, who, false};
  return step_rows(s, K, rows);
}

// ---- the imitation step: gnnb_online_step_rows under the table loss of k_tloss_table ----
// table (DEVICE, (K, R) fp64, row = batch row): what gnnb_strong_pick leaves, NaN where a node is no candidate.  loss (n) fp32, report_i
// (n, 4) int32 [teacher, pick, n_cand, n_viol], regret (n) fp64 and status (int32[1], zeroed by the caller) are DEVICE memory and may be
// NULL.  Synchronises where gnnb_online_step_rows does (repack mode 1 with apply = 1: not at all).
extern "C" int gnnb_imitation_step_rows(gnnb_t* h, const gnnb_batch* in, int K, const int32_t* rows, int n, const double* table, double margin,
                                        float* loss, int32_t* report_i, double* regret, int32_t* status, int apply, void* stream) {
  const char* who = "gnnb_imitation_step_rows";
  if (K < 1 || n < 1 || n > K) return fail(GNNB_E_INVALID, "%s: n = %d rows of a batch of K = %d (1 <= n <= K)", who, n, K);
  if (!(margin >= 0.0)) return fail(GNNB_E_INVALID, "%s: margin = %g (a number >= 0)", who, margin);
  if (!h) return fail(GNNB_E_INVALID, "%s: null handle", who);
  if (!in || !rows || !table) return fail(GNNB_E_INVALID, "%s: null argument", who);
  if (int rc = online_preflight(h, in, K, who)) return rc;
  const StepLoss lf{nullptr, nullptr, table, margin, report_i, regret};
  Step s{h, in, n, lf, StepOut{nullptr, loss, nullptr, status}, apply, (hipStream_t)stream, who, false};
  return step_rows(s, K, rows);
}

// k_tloss_table alone on caller-owned DEVICE arrays (an inspection hook, as gnnb_strong_pick's table is): scores, mask (n, R) fp32, table
// (n, R) fp64, ds (n, R) fp32 zeroed by the caller; loss, report_i, regret, status as above (may be NULL).  Needs a bound handle (for R)
// and no trainer.  Does not synchronise.
extern "C" int gnnb_imitation_loss(gnnb_t* h, const float* scores, const float* mask, const double* table, int n, double margin, float* loss,
                                   float* ds, int32_t* report_i, double* regret, int32_t* status, void* stream) {
  const char* who = "gnnb_imitation_loss";
  if (n < 1) return fail(GNNB_E_INVALID, "%s: n = %d rows (>= 1)", who, n);
  if (!(margin >= 0.0)) return fail(GNNB_E_INVALID, "%s: margin = %g (a number >= 0)", who, margin);
  if (!h) return fail(GNNB_E_INVALID, "%s: null handle", who);
  if (!scores || !mask || !table || !ds) return fail(GNNB_E_INVALID, "%s: null argument", who);
  if (!h->bound) return fail(GNNB_E_STATE, "%s: call gnnb_bind_network first", who);
  hipStream_t st = (hipStream_t)stream;
  gnnb_train::TLossTable la{scores, mask, table, ds, loss, report_i, regret, status, h->R, margin};
  hipLaunchKernelGGL(gnnb_train::k_tloss_table, dim3(n), dim3(256), 0, st, la);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(GNNB_E_HIP, "%s: the launch failed: %s", who, hipGetErrorString(e));
  return GNNB_OK;
}
