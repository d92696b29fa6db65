// CPU-only test shim for gnnb_pack.h (built with g++ by tests/test_pack_cpu.py).  It exposes the operand-order packs and the
// gather tables, so that a numpy emulation of the MFMA lane maps can be checked against a plain matmul / torch conv, and the host
// half of gnnb_bind_network: the layer-list parser with its refusals, the row sums of edge 1, the padded operands of a Linear
// edge, the packed tile table and zero_tap_layer; and check_batch, the one check of a gnnb_batch against a layer graph.
#include "gnnb_pack.h"

static gnnb::Edge conv_edge(const float* w, int c_in, int h_in, int w_in, int c_out, int kh, int kw, int stride, int pad) {
  gnnb::Edge e;
  e.kind = 0; e.c_in = c_in; e.h_in = h_in; e.w_in = w_in; e.c_out = c_out; e.kh = kh; e.kw = kw; e.stride = stride; e.pad = pad;
  e.h_out = (h_in + 2 * pad - kh) / stride + 1; e.w_out = (w_in + 2 * pad - kw) / stride + 1;
  e.n_in = c_in * h_in * w_in; e.n_out = c_out * e.h_out * e.w_out;
  e.w.assign(w, w + (size_t)c_out * c_in * kh * kw);
  return e;
}
static gnnb::Edge linear_edge(const float* w, int n_in, int n_out) {
  gnnb::Edge e{};
  e.kind = 1; e.n_in = n_in; e.n_out = n_out;
  e.w.assign(w, w + (size_t)n_out * n_in);
  return e;
}

extern "C" {
size_t gnnb_pt_blob_floats() { return gnnb::blob_floats(); }
// which: 0 embed, 1 pre_fwd, 2 pre_bwd, 3 pre_inp, 4 prop, 5 upd_fwd_e, 6 upd_fwd_i, 7 upd_fwd_f, 8 upd_bwd, 9 upd_bwd_b,
// 10 upd_inp, 11 post_inp, 12 score_b, 13 score_f
size_t gnnb_pt_pack(const float* blob, int which, float* out, size_t cap) {
  gnnb::Packs pk;
  gnnb::build_packs(blob, pk);
  const std::vector<float>* v[14] = {&pk.embed, &pk.pre_fwd, &pk.pre_bwd, &pk.pre_inp, &pk.prop, &pk.upd_fwd_e, &pk.upd_fwd_i,
                                     &pk.upd_fwd_f, &pk.upd_bwd, &pk.upd_bwd_b, &pk.upd_inp, &pk.post_inp, &pk.score_b, &pk.score_f};
  if (which < 0 || which > 13) return 0;
  if (out && cap >= v[which]->size()) std::memcpy(out, v[which]->data(), v[which]->size() * sizeof(float));
  return v[which]->size();
}

// gather tables for one conv edge.  geom receives 27 ints (see tests/test_pack_cpu.py); returns the
// number of MFMAs per sample, or -1.  cmat / koff are filled when large enough.
long gnnb_pt_gather(const float* w, int c_in, int h_in, int w_in, int c_out, int kh, int kw, int stride, int pad,
                    int dir, int normalise, int allow16, int* geom, float* cmat, size_t cmat_cap, int* koff, size_t koff_cap) {
  const gnnb::Edge e = conv_edge(w, c_in, h_in, w_in, c_out, kh, kw, stride, pad);
  gnnb::GatherHost g;
  if (!gnnb::build_gather(e, dir, normalise != 0, g, 0, allow16 != 0)) return -1;
  const gnnb::GatherGeom& q = g.g;
  const int v[27] = {q.tm.N, q.tm.C, q.tm.H, q.tm.W, q.tm.CT, q.tm.PY, q.tm.PX, q.tm.ay, q.tm.ax, q.tm.NBY, q.tm.NBX, q.tm.NCG,
                     q.tm.TPS, q.K2, q.Hs, q.Ws, q.Ns, q.ystep, q.ybase, q.xstep, q.xbase, q.WY, q.WX, q.normalise,
                     (int)g.cmat.size(), (int)g.koff.size(), q.lanes};
  for (int i = 0; i < 27; ++i) geom[i] = v[i];
  if (cmat && cmat_cap >= g.cmat.size()) std::memcpy(cmat, g.cmat.data(), g.cmat.size() * sizeof(float));
  if (koff && koff_cap >= g.koff.size()) std::memcpy(koff, g.koff.data(), g.koff.size() * sizeof(int));
  return g.mfma_per_sample;
}

// parse_layers.  Returns the number of graph layers (N, relu_q, hw filled when cap holds them; rn = {R, n_fixed}), or -1 with the
// refusal in err.
int gnnb_pt_parse(const gnnb_layer_desc* L, int n, int c0, int h0, int w0, int* N, int* relu_q, int* hw, int cap, int* rn, char* err, size_t err_cap) {
  gnnb::LayerGraph g;
  const std::string refusal = gnnb::parse_layers(L, n, c0, h0, w0, g);
  if (!refusal.empty()) {
    snprintf(err, err_cap, "%s", refusal.c_str());
    return -1;
  }
  const int K = (int)g.N.size();
  for (int k = 0; k < K && K <= cap; ++k) {
    N[k] = g.N[k];
    if (k < K - 1) { relu_q[k] = g.relu_q[k]; hw[k] = g.hw[k]; }
  }
  rn[0] = g.R; rn[1] = g.n_fixed;
  return K;
}

// check_batch of `in` against a layer list parse_layers accepts, with the needs of entry point `which` (0 gnnb_forward, 1 gnnb_forward_host,
// 2 gnnb_pack_amb_records, 3 gnnb_online_step): 1 accepted, 0 refused with the refusal in err, -1 the list is refused
int gnnb_pt_check_batch(const gnnb_layer_desc* L, int n, int c0, int h0, int w0, const gnnb_batch* in, int B, int which, char* err, size_t err_cap) {
  gnnb::LayerGraph g;
  if (which < 0 || which > 3 || !gnnb::parse_layers(L, n, c0, h0, w0, g).empty()) return -1;
  const gnnb::BatchNeeds needs[4] = {gnnb::kNeedsForward, gnnb::kNeedsForwardHost, gnnb::kNeedsPack, gnnb::kNeedsOnline};
  const std::string refusal = gnnb::check_batch(g, *in, B, needs[which]);
  snprintf(err, err_cap, "%s", refusal.c_str());
  return refusal.empty() ? 1 : 0;
}

// zero_tap_layer of a layer list parse_layers accepts: the layer (0: none), yx = one of its unread pixels; -1: the list is refused
int gnnb_pt_zero_tap(const gnnb_layer_desc* L, int n, int c0, int h0, int w0, int* yx) {
  gnnb::LayerGraph g;
  if (!gnnb::parse_layers(L, n, c0, h0, w0, g).empty()) return -1;
  return gnnb::zero_tap_layer(g, &yx[0], &yx[1]);
}

// edge1_row_sums of a conv (kind 0; n_out = c_out * h_out * w_out sums) or a Linear n_in -> n_out (kind 1, w (n_out, n_in)); returns their number
int gnnb_pt_row_sums(const float* w, int kind, int c_in, int h_in, int w_in, int c_out, int kh, int kw, int stride, int pad, int n_in, int n_out,
                     float* out) {
  const gnnb::Edge e = kind == 0 ? conv_edge(w, c_in, h_in, w_in, c_out, kh, kw, stride, pad) : linear_edge(w, n_in, n_out);
  const std::vector<float> s = gnnb::edge1_row_sums(e);
  std::memcpy(out, s.data(), s.size() * sizeof(float));
  return (int)s.size();
}

// dense_operands of a Linear n_in -> n_out.  geom: ld_fwd, mt_fwd, ksq_fwd, ld_bwd, mt_bwd, ksq_bwd, kpad_fwd, kpad_bwd, then the floats
// of the forward and of the transposed image (copied when the caps hold them).
void gnnb_pt_dense(const float* w, int n_in, int n_out, int* geom, float* fwd, size_t fwd_cap, float* bwd, size_t bwd_cap) {
  const gnnb::DenseHost d = gnnb::dense_operands(linear_edge(w, n_in, n_out));
  const int v[10] = {d.g.ld_fwd, d.g.mt_fwd, d.g.ksq_fwd, d.g.ld_bwd, d.g.mt_bwd, d.g.ksq_bwd, d.g.kpad_fwd, d.g.kpad_bwd, (int)d.fwd.size(), (int)d.bwd.size()};
  for (int i = 0; i < 10; ++i) geom[i] = v[i];
  if (fwd && fwd_cap >= d.fwd.size()) std::memcpy(fwd, d.fwd.data(), d.fwd.size() * sizeof(float));
  if (bwd && bwd_cap >= d.bwd.size()) std::memcpy(bwd, d.bwd.data(), d.bwd.size() * sizeof(float));
}

// tile_table of a tile map of NCG x NBY x NBX tiles: 1 and the NCG * NBY * NBX words in out, or 0 where a field overflows
int gnnb_pt_tile_table(int NCG, int NBY, int NBX, int* out) {
  gnnb::TileMap tm;
  tm.NCG = NCG; tm.NBY = NBY; tm.NBX = NBX; tm.TPS = NCG * NBY * NBX;
  std::vector<int> tt;
  if (!gnnb::tile_table(tm, tt)) return 0;
  std::memcpy(out, tt.data(), tt.size() * sizeof(int));
  return 1;
}
}
