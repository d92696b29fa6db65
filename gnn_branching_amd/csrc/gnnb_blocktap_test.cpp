// CPU-only test shim for the block-form tap image of gnnb_pack.h (blocktap_ok / blocktap_image), built with g++ by tests/test_blocktap_cpu.py.
// With -DBLOCKTAP_MAIN it is a stand-alone program that builds the tables of a few first convolutions and checks every entry of the image
// against the weight it must hold (for a run under -fsanitize=address,undefined):
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -DBLOCKTAP_MAIN -o blocktap_test gnnb_blocktap_test.cpp && ./blocktap_test
#include "gnnb_pack.h"

static gnnb::Edge bt_conv_edge(const float* w, int c_in, int h_in, int w_in, int c_out, int kh, int kw, int stride, int pad) {
  gnnb::Edge e;
  e.kind = 0; e.c_in = c_in; e.h_in = h_in; e.w_in = w_in; e.c_out = c_out; e.kh = kh; e.kw = kw; e.stride = stride; e.pad = pad;
  e.h_out = (h_in + 2 * pad - kh) / stride + 1; e.w_out = (w_in + 2 * pad - kw) / stride + 1;
  e.n_in = c_in * h_in * w_in; e.n_out = c_out * e.h_out * e.w_out;
  e.w.assign(w, w + (size_t)c_out * c_in * kh * kw);
  return e;
}

extern "C" {
// The forward tables of one conv edge as bind builds them for edge 1.  geom: {lanes, CT, PY, PX, NCG, K2, WY, WX, ncy}.  Returns 1 where
// the edge takes the block form (img receives blocktap_image when it fits), 0 where it keeps the 16-column form, -1 without tables.
int gnnb_bt_image(const float* w, int c_in, int h_in, int w_in, int c_out, int kh, int kw, int stride, int pad, int* geom, float* img, size_t cap) {
  const gnnb::Edge e = bt_conv_edge(w, c_in, h_in, w_in, c_out, kh, kw, stride, pad);
  gnnb::GatherHost g;
  if (!gnnb::build_gather(e, 0, false, g, 0, true)) return -1;
  const bool ok = gnnb::blocktap_ok(e, 0, g.g);
  const int v[9] = {g.g.lanes, g.g.tm.CT, g.g.tm.PY, g.g.tm.PX, g.g.tm.NCG, g.g.K2, g.g.WY, g.g.WX, ok ? gnnb::blocktap_rows(e) : 0};
  for (int i = 0; i < 9; ++i) geom[i] = v[i];
  if (!ok) return 0;
  const std::vector<float> im = gnnb::blocktap_image(e, g.g);
  if (img && cap >= im.size()) std::memcpy(img, im.data(), im.size() * sizeof(float));
  return 1;
}
}

#ifdef BLOCKTAP_MAIN
#include <cstdio>
int main() {
  struct Case { int c_in, h, w, c_out, k, s, p; } cases[] = {{3, 32, 32, 8, 4, 2, 1}, {3, 32, 32, 16, 4, 2, 1}, {3, 34, 10, 8, 4, 2, 1}, {3, 4, 4, 8, 4, 2, 1},
                                                               {3, 12, 20, 8, 5, 1, 2}};
  int taken = 0;
  for (const Case& c : cases) {
    std::vector<float> w((size_t)c.c_out * c.c_in * c.k * c.k);
    for (size_t i = 0; i < w.size(); ++i) w[i] = 1.0f + (float)i;
    int geom[9];
    std::vector<float> img((size_t)c.c_out / 8 * 12 * 64 + 64, -1.0f);
    const int r = gnnb_bt_image(w.data(), c.c_in, c.h, c.w, c.c_out, c.k, c.k, c.s, c.p, geom, img.data(), img.size());
    printf("conv %d -> %d, %dx%d/%d/%d on %dx%d: tile [%d, %d, %d] of %d lanes, %s\n", c.c_in, c.c_out, c.k, c.k, c.s, c.p, c.h, c.w, geom[1], geom[2], geom[3],
           geom[0], r == 1 ? "block form" : r == 0 ? "16-column form" : "no tables");
    if (r != 1) continue;
    ++taken;
    for (int cg = 0; cg < geom[4]; ++cg)
      for (int cy = 0; cy < geom[8]; ++cy)
        for (int pg = 0; pg < 4; ++pg)
          for (int col = 0; col < 4; ++col)
            for (int kx = 0; kx < 4; ++kx) {
              const int co = cg * 8 + 4 * (pg & 1) + col, cs = cy / c.k, ky = cy % c.k;
              const float want = w[(((size_t)co * c.c_in + cs) * c.k + ky) * c.k + kx];
              if (img[(((size_t)cg * geom[8] + cy) * 4 + pg) * 16 + col * 4 + kx] != want) { printf("image mismatch\n"); return 1; }
            }
  }
  if (taken != 2) { printf("expected exactly the two [8, 1, 2] tilings to take the block form\n"); return 1; }
  printf("ok\n");
  return 0;
}
#endif
