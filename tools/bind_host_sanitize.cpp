// dev helper: the host half of gnnb_bind_network (gnnb_pack.h) under AddressSanitizer + UBSan, as a stand-alone CPU program.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -DGNNB_PACK_NO_THREADS \
//       -o /tmp/bind_host_sanitize tools/bind_host_sanitize.cpp && /tmp/bind_host_sanitize
// It parses one accepted and one refused layer list and builds the row sums of edge 1, the dense operands of a 65 -> 33 Linear
// edge, a tile table, the zero-tap scan and the fp64 kernels' geometry, and runs check_batch on an accepted batch and on one refusal of
// each kind (batch size, count, null table, null entry, null loose pointer).  Exit status 0 and "ok" when nothing was flagged.
#include <cstdio>

#include "../gnn_branching_amd/csrc/gnnb_pack.h"

struct Net {      // the members fill_kw_geometry writes (gnnb_k_kw.h KwNet without its device pointers)
  gnnb::EdgeGeom e[gnnb::kMaxReluLayers + 2];
  int N[gnnb::kMaxReluLayers + 2], off[gnnb::kMaxReluLayers + 2], lc[gnnb::kMaxReluLayers + 2], lh[gnnb::kMaxReluLayers + 2], lw[gnnb::kMaxReluLayers + 2];
  int L, R, maxNr;
};

int main() {
  using namespace gnnb;
  std::vector<float> w1(8 * 3 * 4 * 4, 0.25f), b1(8, 0.f), w2(33 * 128, -0.5f), b2(33, 0.f);
  gnnb_layer_desc conv{}, relu{}, flat{}, lin{};
  conv.kind = GNNB_CONV; conv.c_in = 3; conv.c_out = 8; conv.kh = conv.kw = 4; conv.stride = 2; conv.pad = 1;
  conv.weight = w1.data(); conv.bias = b1.data();
  relu.kind = GNNB_RELU;
  flat.kind = GNNB_FLATTEN;
  lin.kind = GNNB_LINEAR; lin.n_in = 128; lin.n_out = 33; lin.weight = w2.data(); lin.bias = b2.data();
  const gnnb_layer_desc good[] = {conv, relu, flat, lin, relu}, bad[] = {conv, relu, flat, lin, lin, relu};
  LayerGraph g, none;
  const std::string ok = parse_layers(good, 5, 3, 8, 8, g), refusal = parse_layers(bad, 6, 3, 8, 8, none);
  if (!ok.empty() || refusal != "layer 4: two linear maps without a ReLU between them" || g.N.size() != 4 || g.R != 128 + 33) return 1;
  const std::vector<float> s1 = edge1_row_sums(g.edges[1]);
  Edge e{};
  e.kind = 1; e.n_in = 65; e.n_out = 33;
  e.w.assign((size_t)65 * 33, 1.f);
  const DenseHost d = dense_operands(e);
  GatherHost gh;
  std::vector<int> tt;
  if (!build_gather(g.edges[1], 1, false, gh, 132, true) || !tile_table(gh.g.tm, tt)) return 2;
  int y = 0, x = 0;
  const int zk = zero_tap_layer(g, &y, &x);
  Net net;
  fill_kw_geometry(net, g);
  // check_batch: N = {192, 128, 33, 1}, five fixed layers -> 4 bound, 2 dual, 6 primal tensors; the checker looks at no tensor's memory
  const float f = 0.f;
  const float *four[4] = {&f, &f, &f, &f}, *two[2] = {&f, &f}, *six[6] = {&f, &f, &f, &f, &f, &f}, *hole[6] = {&f, &f, nullptr, &f, &f, &f},
              *gap[6] = {&f, nullptr, &f, &f, &f, &f};
  const gnnb_batch fine{four, four, two, six, &f, &f, &f, &f, 4, 2, 6};
  gnnb_batch count = fine, tab = fine, unread = fine, entry = fine, loose = fine;
  count.n_relu = 1; tab.dual = nullptr; unread.primal = hole; entry.primal = gap; loose.mask = nullptr;
  const std::string verdicts[] = {check_batch(g, fine, 2, kNeedsForward), check_batch(g, fine, 0, kNeedsForward), check_batch(g, count, 2, kNeedsPack),
                                  check_batch(g, tab, 2, kNeedsForwardHost), check_batch(g, unread, 2, kNeedsForward),
                                  check_batch(g, unread, 2, kNeedsForwardHost), check_batch(g, entry, 2, kNeedsOnline),
                                  check_batch(g, loose, 2, kNeedsOnline), check_batch(g, loose, 2, kNeedsPack)};
  const bool accepted[] = {true, false, false, false, false, true, false, false, true};
  for (int i = 0; i < 9; ++i) {
    printf("check_batch %d: %s\n", i, verdicts[i].empty() ? "accepted" : verdicts[i].c_str());
    if (verdicts[i].empty() != accepted[i]) return 4;
  }
  printf("ok: %zu row sums (corner %g, centre %g), dense images %zu + %zu floats, %zu tiles, zero-tap layer %d, widest ReLU layer %d\n",
         s1.size(), s1[0], s1[5], d.fwd.size(), d.bwd.size(), tt.size(), zk, net.maxNr);
  return s1.size() == 128 && zk == 0 && net.maxNr == 128 ? 0 : 3;
}
